"""The PINNED fp64 engine (PPCA_GRAM_FP64=1: the `mode == 1` branch of launch_pass_guarded, pass_kernel<K, EM, false> without
qprep, guard or reduction verdict) against the oracle.  The other tests reach the fp64 instantiations only behind a tripped guard.
The variable is read once when the library loads, so the library runs in a fresh child process (this file as a script)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

CASES = [(256, 10, False), (37, 3, False), (64, 1, True)]  # (d, k, weighted)
N = 5 * 32 + 7  # several tiles and a ragged last one


def _case(d, k, weighted):
    """-> x (30 % masked, one row without an observed entry), w or None, and a model (sigma, C, mean)."""
    rng = np.random.default_rng(1000 * d + k)
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.6
    x = rng.standard_normal((N, k)) @ (0.7 * rng.standard_normal((k, d))) + 0.3 * rng.standard_normal((N, d))
    x[rng.random((N, d)) < 0.3] = np.nan
    x[N // 2] = np.nan
    return x, (rng.uniform(0.25, 2.0, N) if weighted else None), s, c, mu


def _child(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ppca_rs_amd as P
    from ppca_rs_amd import _lib

    out = {}
    for d, k, weighted in CASES:
        x, w, s, c, mu = _case(d, k, weighted)
        ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
        eng = C.c_int32(-1)
        _lib.check(_lib.lib().ppca_gram_engine(ds._ctx.handle, m._device(ds._ctx).h, C.byref(eng)))
        new, inf = m.iterate(ds), m.infer(ds)
        out.update({f"{d}_{k}_{name}": np.asarray(v) for name, v in (
            ("engine", eng.value), ("sigma", new.isotropic_noise), ("c", new.transform), ("mean", new.mean), ("llks", m.llks(ds)),
            ("states", inf.states()), ("covs", np.array(inf.covariances())), ("smooth", m.smooth(ds).numpy()))})
    np.savez(path, **out)
    print("pinned fp64 child written")


@pytest.mark.gpu
def test_pinned_fp64_engine_matches_oracle(hiplib, oracle, tmp_path):
    """One iterate, llks, infer with covariances and smooth per case, every array finite and within the bounds that
    test_gpu_parity.py's test_int8_gram_dynamic_range_guard holds the same quantities to on the fp64 engine after one step, written
    in that file's RTOL: 1e-8 = RTOL * 1e-3 for the new model (sigma, transform, mean), 1e-9 = RTOL * 1e-4 for llks and states.
    Smooth is held to 1e-9 and the covariances to 1e-8 as in test_golden (that test's 1e-6 for the covariances belongs to its
    ill-conditioned model).  Measured on these well-conditioned cases: every figure below 1e-13."""
    from test_gpu_parity import RTOL, _rel

    path = str(tmp_path / "pinned.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True,
                       env=dict(os.environ, PPCA_GRAM_FP64="1"), timeout=300)
    assert r.returncode == 0 and "pinned fp64 child written" in r.stdout, (r.stdout[-1500:], r.stderr[-2500:])
    got = np.load(path)
    for d, k, weighted in CASES:
        x, w, s, c, mu = _case(d, k, weighted)
        g = {name: got[f"{d}_{k}_{name}"] for name in ("engine", "sigma", "c", "mean", "llks", "states", "covs", "smooth")}
        for name, v in g.items():
            assert np.isfinite(v).all(), (d, k, name)
        assert int(g["engine"]) == 1, (d, k)
        s1, c1, m1 = oracle.iterate(x, s, c, mu, w)
        st, cv = oracle.infer(x, s, c, mu)
        err = {"sigma": abs(float(g["sigma"]) - s1) / s1, "c": _rel(g["c"], c1), "mean": _rel(g["mean"], m1),
               "llks": _rel(g["llks"], oracle.llks(x, s, c, mu)), "states": _rel(g["states"], st), "covs": _rel(g["covs"], cv),
               "smooth": _rel(g["smooth"], oracle.reconstruct(x, s, c, mu, "smooth"))}
        print((d, k), {name: "%.2e" % e for name, e in err.items()})
        assert err["sigma"] < RTOL * 1e-3 and err["c"] < RTOL * 1e-3 and err["mean"] < RTOL * 1e-3, (d, k, err)
        assert err["llks"] < RTOL * 1e-4 and err["states"] < RTOL * 1e-4 and err["smooth"] < RTOL * 1e-4, (d, k, err)
        assert err["covs"] < RTOL * 1e-3, (d, k, err)


if __name__ == "__main__":
    _child(sys.argv[1])
