"""Cases of the split pipeline (ppca_generic.hip + ppca_solve4.hip) whose branch is chosen by a variable the library reads ONCE per
process, so that they need a process of their own; tests/test_gpu_split_steady_state.py runs this file as a child and compares what it
wrote with the oracle (and, for the addressing form, bit for bit with a second child).

    python tools/split_check.py MODE OUT.npz

    MODE ptr     three shapes of the int8 GEMM (128-row tile, 256-row tile, XCD-aware tile order, a product cut along the samples);
                 run once as it is and once under PPCA_I8GEMM_PTR=1 (operands by pointer arithmetic, the form for >= 2 GiB)
    MODE fp64    under PPCA_GENERIC_FP64=1: both large contractions on the fp64 MFMA, the statistics product cut along K; every output
                 pass as well (their Gram is then the unguarded fp64 product)
    MODE chunks  under PPCA_GEN_CHUNK=16448: three chunks of more than 16 384 rows, once with weights that grow by 2^20 from chunk to
                 chunk (every column of a later chunk is cut a second time, by a grid capped along the rows) and once with ordinary
                 weights (every chunk weighs the same in the sums); the scalars and outputs of an output pass across chunks
    MODE inert   under every RETIRED switch of the split pipeline at its non-default value (the test holds the list): the smallest
                 shapes at which each of them used to change the route; one EM statistics pass and one smooth pass each

Writes, per case NAME: NAME_stats (ppca_stats_raw), NAME_trace (ppca_generic_last_trace of that pass, as JSON) and what the mode adds.
The inputs are not written: case_data() makes them again from the case's seed."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CASES = {
    # name: (seed, n, d, k, weighted)
    "ptr": {"sliced": (11, 8192 + 37, 300, 4, True), "xcd": (12, 1500, 70, 33, False), "tall": (13, 1300, 1100, 20, True)},
    "fp64": {"k4": (21, 2100, 300, 4, True), "k20": (23, 2100, 70, 20, True), "k40": (22, 2100, 70, 40, False)},
    "chunks": {"grow": (31, 2 * 16448 + 16400, 260, 3, True), "flat": (32, 2 * 16448 + 16400, 260, 3, True)},
    "inert": {"lane": (41, 600, 300, 8, True), "solve4": (42, 4200, 70, 32, False), "tall": (43, 600, 1024, 4, True),
              "mfma": (44, 300, 70, 70, True)},
}
CHUNK = 16448


def case_data(mode, name):
    """x (n x d, NaN = masked, one all-masked row), weights (or None), (sigma, C, mean) of a case."""
    seed, n, d, k, weighted = CASES[mode][name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, k)) @ rng.standard_normal((k, d)) + 0.2 * rng.standard_normal((n, d)) + rng.standard_normal(d)
    x[rng.random((n, d)) < 0.35] = np.nan
    x[n // 3] = np.nan
    w = rng.uniform(0.5, 2.0, n) if weighted else None
    if name == "grow":
        for c in range(1, (n + CHUNK - 1) // CHUNK):
            w[c * CHUNK:] *= 2.0 ** 20
    m = (0.4 + rng.random(), 0.5 * rng.standard_normal((d, k)), 0.3 * rng.standard_normal(d))
    return x, w, m


def main():
    import ppca_rs_amd as P
    from ppca_rs_amd import _lib

    mode, path = sys.argv[1], sys.argv[2]
    ctx = _lib.default_context()
    out = {}
    for name in CASES[mode]:
        x, w, m = case_data(mode, name)
        d, k = m[1].shape
        assert _lib.lib().ppca_path_kind(d, k) == 0
        ds, mod = P.Dataset(x, w), P.PPCAModel(*m)
        st = np.empty(_lib.lib().ppca_stats_len(d, k))
        _lib.check(_lib.lib().ppca_stats_raw(ctx.handle, ds._h, mod._device(ctx).h, _lib.ptr(st)))
        out[name + "_stats"], out[name + "_trace"] = st, json.dumps(ctx.generic_trace())
        if mode in ("fp64", "chunks"):
            out[name + "_llks"], out[name + "_llk"] = mod.llks(ds), mod.llk(ds)
            out[name + "_trace_llk"] = json.dumps(ctx.generic_trace())
        if mode in ("chunks", "inert"):
            out[name + "_smooth"] = mod.smooth(ds).numpy()
            out[name + "_trace_smooth"] = json.dumps(ctx.generic_trace())
        if mode == "fp64":
            inf = mod.infer(ds)
            out[name + "_trace_infer"] = json.dumps(ctx.generic_trace())
            out[name + "_states"], out[name + "_covs"] = inf.states(), np.array(inf.covariances())
            out[name + "_smooth"], out[name + "_extrapolate"] = mod.smooth(ds).numpy(), mod.extrapolate(ds).numpy()
            for mode_id, what in ((0, "smooth"), (1, "extrapolate")):
                h = C.c_void_p()
                _lib.check(_lib.lib().ppca_covariance_diagonal(ctx.handle, ds._h, mod._device(ctx).h, mode_id, C.byref(h)))
                out[name + "_diag_" + what] = P.Dataset._wrap(h, ctx).numpy()
    np.savez(path, **out)
    print("split check written", path)


if __name__ == "__main__":
    main()
