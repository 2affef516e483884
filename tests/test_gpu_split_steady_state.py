"""The SIZE-GATED branches of the split pipeline (ppca_generic.hip + ppca_solve4.hip) under the oracle.

The host side of the split pipeline chooses kernel variants, tiles, addressing forms, K-splits and persistent grids by thresholds on
N, d, k and the CU count; at the sizes the CPU oracle affords (n <= ~4000 on 256 CUs) every other oracle test takes the small-N side
of nearly all of them.  Here `ppca_ctx_set_grid_limit` (or the size itself, where the oracle can pay for it) puts a case on the
large-N side, every block of the statistics / every output is compared with the oracle, and the case ASSERTS through the host's
dispatch record (`ppca_generic_last_trace`, Context.generic_trace()) that the branch it exists for ran -- a retuned threshold makes it
fail with "branch not reached" instead of quietly shrinking what is covered.

Branches (numbers as in the tests' names and messages):
  1  the int8 statistics product cut along the samples (I8GemmArgs::ksplit / nsplit / out2, add_partial_kernel)
  2  "the last column blocks cut along the samples": the pair of launches with offset operand, scale and output pointers
  3  the fp64 GEMM cut along K (launch_gemm with scratch, splitk_reduce_kernel): k >= 80, a chunk whose S guard trips, PPCA_GENERIC_FP64=1
  4  skinny_xt_kernel with many slices, all five column-tile instantiations, a short last slice
  5  the persistent loops of the per-sample solvers (lane, solve4, one sample per wave on the MFMA) past their first iteration
  6  gen_wdigits_kernel re-cutting columns with its grid capped along the rows
  7  recon2_kernel with more than 16 rows per block and two blocks along the dimensions
  8  scal_reduce_kernel / scal_final_kernel with many blocks, accumulating across the chunks of an output pass
  9  the int8 GEMM addressing its operands by pointer arithmetic (PPCA_I8GEMM_PTR=1)

Tolerances are those of tests/test_gpu_parity.py::test_generic_pipeline_matches_oracle for these shapes: 1e-8 statistics blocks, 1e-9
log-likelihoods, 1e-7 states and covariances (and the covariance diagonals, which are functions of them), 1e-8 reconstructions.  Every case: one all-masked row and n no
multiple of 64; d no multiple of 64 except where the shape is the point (configuration 4's d = 1024; d = 256 and 64 among the output
passes of k = 11..16)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_STATS, TOL_LLK, TOL_STATE, TOL_RECON = 1e-8, 1e-9, 1e-7, 1e-8
LANE, LANE_WIDE, SOLVE4, MFMA = 1, 2, 3, 4  # ppca_generic_trace::solver


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@pytest.fixture()
def ctx(P):
    from ppca_rs_amd import _lib

    c = _lib.default_context()
    c.set_grid_limit(0)
    yield c
    c.set_grid_limit(0)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _blocks(d, k):
    kp = k * (k + 1) // 2
    b = [0, d * k, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d, 2 * d * k + d * kp + 2 * d]
    return list(zip(["cross", "S", "U", "sumx", "totals", "scalars"], b, b[1:] + [b[-1] + 8]))


def _stats(ctx, ds, m, fused16=0):
    """(ppca_stats_raw, the dispatch record of that pass); fused16 = 1: the pass is expected on the two-kernel pass of k = 11..16"""
    from ppca_rs_amd import _lib

    got = np.empty(_lib.lib().ppca_stats_len(m.output_size, m.state_size))
    _lib.check(_lib.lib().ppca_stats_raw(ctx.handle, ds._h, m._device(ctx).h, _lib.ptr(got)))
    t = ctx.generic_trace()
    assert t["valid"] == 1 and t["em"] == 1 and t["fused16"] == fused16 and (t["d"], t["k"], t["n"]) == (m.output_size, m.state_size, len(ds)), t
    return got, t


def _assert_stats(got, want, d, k, tag):
    for name, a, b in _blocks(d, k):
        err = _rel(got[a:b], want[a:b])
        print("stats", tag, name, "%.2e" % err)
        assert err < TOL_STATS, (name, err) + tuple(tag)


def _masked_diag_of_S(got, want, x, row, d, k):
    """S_j's diagonal, dimension by dimension where `row` is masked (tests/test_gpu_steady_state.py::test_outlier_row_on_the_split_pipeline)"""
    kp = k * (k + 1) // 2
    diag = [a * (a + 1) // 2 + a for a in range(k)]
    Sg, Sw = got[d * k:d * k + d * kp].reshape(d, kp), want[d * k:d * k + d * kp].reshape(d, kp)
    masked = ~np.isfinite(x[row])
    assert masked.any()
    return (np.abs(Sg[masked][:, diag] - Sw[masked][:, diag]) / np.abs(Sw[masked][:, diag])).max()


def _case(oracle, n, d, k, seed, weighted=True, mask=0.3):
    rng = np.random.default_rng(seed)
    x, _, _ = oracle.synth(n, d, k, mask, 9000 + seed)
    x[n // 3] = np.nan  # an all-masked row
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.7
    w = rng.uniform(0.25, 2.0, n) if weighted else None
    return x, w, (s, c, mu)


def _post_against_oracle(P, oracle, ctx, x, w, model, tag, expect=None):
    """Every output pass (generic_post) against the oracle; `expect(trace, what)` after each pass.  Returns the traces by pass."""
    from ppca_rs_amd import _lib

    s, c, mu = model
    m, ds = P.PPCAModel(s, c, mu), P.Dataset(x, w)
    traces = {}

    def seen(what):
        t = ctx.generic_trace()
        assert t["valid"] == 1 and t["em"] == 0 and t["n"] == len(x), (what, t)
        traces[what] = t
        if expect:
            expect(t, what)

    err = _rel(m.llks(ds), oracle.llks(x, s, c, mu))
    seen("llks")
    print("post", tag, "llks %.2e" % err)
    assert err < TOL_LLK, (tag, err)
    want = oracle.llk(x, s, c, mu, w)
    assert abs(m.llk(ds) - want) < TOL_LLK * abs(want), tag
    seen("llk")
    st, cv = oracle.infer(x, s, c, mu)
    inf = m.infer(ds)
    seen("infer")
    e1, e2 = _rel(inf.states(), st), _rel(np.array(inf.covariances()), cv)
    print("post", tag, "states %.2e covariances %.2e" % (e1, e2))
    assert e1 < TOL_STATE and e2 < TOL_STATE, (tag, e1, e2)
    del inf, cv
    err = _rel(m.smooth(ds).numpy(), oracle.reconstruct(x, s, c, mu, "smooth"))
    seen("smooth")
    print("post", tag, "smooth %.2e" % err)
    assert err < TOL_RECON, (tag, err)
    ex = m.extrapolate(ds).numpy()
    seen("extrapolate")
    err = _rel(ex, oracle.reconstruct(x, s, c, mu, "extrapolate"))
    print("post", tag, "extrapolate %.2e" % err)
    assert err < TOL_RECON, (tag, err)
    assert np.array_equal(ex[np.isfinite(x)], x[np.isfinite(x)]), tag  # observed entries: bit-exact
    for mode, name in ((0, "smooth"), (1, "extrapolate")):
        h = C.c_void_p()
        _lib.check(_lib.lib().ppca_covariance_diagonal(ctx.handle, ds._h, m._device(ctx).h, mode, C.byref(h)))
        seen("diag_" + name)
        err = _rel(P.Dataset._wrap(h, ctx).numpy(), oracle.covariance_diagonal(x, s, c, mu, name))
        print("post", tag, "diagonal", name, "%.2e" % err)
        assert err < TOL_STATE, (tag, name, err)  # (c_j^T Sigma c_j: a function of the covariances, held to their bound)
    return traces


def _stat_launches(t):
    return [g for g in t["i8gemm"] if g["role"] != 0]


# ------------------------------------------------------------------ branch 1
@pytest.mark.parametrize("k", [4, 10])
def test_statistics_product_cut_along_the_samples(P, oracle, ctx, k):
    """Branch 1.  d = 300: three row blocks x one or two column blocks leave the chip idle, so the int8 statistics product is cut into
    slices of >= 4096 samples whose partials add_partial_kernel sums in slice order.  n = 8192 + 37 (two slices) and n = 19 999 (four on
    the full grid, fewer on a capped one), weighted and not."""
    d = 300
    seen = set()
    for n in (8192 + 37, 19_999):
        x, w, (s, c, mu) = _case(oracle, n, d, k, 100 + k + n % 7)
        m = P.PPCAModel(s, c, mu)
        for weights in (w, None):
            want = oracle.stats(x, s, c, mu, weights)
            for cap in (0, 4):
                ctx.set_grid_limit(cap)
                got, t = _stats(ctx, P.Dataset(x, weights), m)
                (sl,) = _stat_launches(t)
                print("branch 1", (k, n, cap), sl, "chunks", t["chunks"])
                assert t["stats_sliced"] == 1 and sl["role"] == 1 and sl["nsplit"] >= 2, ("branch 1 not reached", k, n, cap, t)
                seen.add(sl["nsplit"])
                _assert_stats(got, want, d, k, (k, n, cap, weights is None))
    assert len(seen) >= 2 and max(seen) > 2, ("branch 1: one slice count only", seen)


# ------------------------------------------------------------------ branch 2
def test_last_column_block_pair_at_config4_shape(P, oracle, ctx):
    """Branch 2 on the FULL grid at BASELINE configuration 4's shape (d = 1024, k = 64, half of every row masked as one cyclic run):
    65 column blocks x 4 row blocks of 256 rows -- 64 column blocks run whole, the last is cut along the samples.  EM statistics only
    (the oracle takes about a minute for them)."""
    n, d, k = 8192 + 101, 1024, 64
    rng = np.random.default_rng(d + k)
    x, _, _ = oracle.synth(n, d, k, 0.0, 700 + d)
    starts = rng.integers(0, d, n)
    cols = (starts[:, None] + np.arange(d // 2)[None, :]) % d
    x[np.arange(n)[:, None], cols] = np.nan
    x[1] = np.nan
    w = rng.uniform(0.5, 1.5, n)
    c, mu, s = 0.3 * rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d), 0.9
    got, t = _stats(ctx, P.Dataset(x, w), P.PPCAModel(s, c, mu))
    head, tail = _stat_launches(t)
    print("branch 2 (config 4)", head, tail, "n_cu", t["n_cu"])
    assert t["stats_pair"] == 1 and (head["role"], tail["role"]) == (2, 3) and tail["nsplit"] >= 2, ("branch 2 not reached", t)
    assert head["tile_rows"] == 256 and tail["tile_rows"] == 256 and head["xcd_map"] == 1 and head["nsplit"] == 1, t
    _assert_stats(got, oracle.stats(x, s, c, mu, w), d, k, ("config 4",))


def test_last_column_block_pair_under_a_grid_limit(P, oracle, ctx):
    """Branch 2 at a cheap shape: d = 300, k = 24 on 14 "CUs" -- 28 slots, 3 row blocks x 10 column blocks, nine column blocks in one
    round and the tenth cut along the samples; weighted and not.  Then the same with one row x 1e6: the chunk's S guard trips, the int8
    launches return at once and the fp64 product behind the same partial scratch is the one that counts (branch 3: cut along K) -- S
    dimension by dimension where that row is masked, as test_outlier_row_on_the_split_pipeline."""
    n, d, k = 8192 + 37, 300, 24
    x, w, (s, c, mu) = _case(oracle, n, d, k, 24)
    m = P.PPCAModel(s, c, mu)
    ctx.set_grid_limit(14)
    for weights in (w, None):
        got, t = _stats(ctx, P.Dataset(x, weights), m)
        head, tail = _stat_launches(t)
        print("branch 2 (limit 14)", head, tail)
        assert t["stats_pair"] == 1 and (head["role"], tail["role"]) == (2, 3) and tail["nsplit"] >= 4, ("branch 2 not reached", t)
        _assert_stats(got, oracle.stats(x, s, c, mu, weights), d, k, ("limit 14", weights is None))
    xo = x.copy()
    xo[100] *= 1e6
    got, t = _stats(ctx, P.Dataset(xo, w), m)
    g2 = [g for g in t["gemm"] if g["amode"] == 2 and g["guarded"]]
    print("branch 2 + 3 (guard trips)", _stat_launches(t), g2)
    assert t["stats_pair"] == 1 and len(g2) == 1 and g2[0]["kslices"] >= 2, ("branch 3 (guarded) not reached", t)
    want = oracle.stats(xo, s, c, mu, w)
    _assert_stats(got, want, d, k, ("limit 14", "outlier"))
    err = _masked_diag_of_S(got, want, xo, 100, d, k)
    print("masked diagonal of S %.2e" % err)
    assert err < 1e-9  # (the int8 form alone: 1e-5 and worse -- what passes here came from the fp64 product)


# ------------------------------------------------------------------ branch 3
@pytest.mark.parametrize("k,d,n", [(80, 150, 1100), (100, 140, 1500), (128, 150, 1100)])
def test_fp64_products_cut_along_k_at_large_state_sizes(P, oracle, ctx, k, d, n):
    """Branch 3.  k >= 80: k + 1 columns are more than the skinny kernel takes, so [U | totals] and [cross | sumx] go through
    gemm_kernel<2> / <3>, cut along the samples once there are >= 512 of them (the output passes have no such product)."""
    x, w, model = _case(oracle, n, d, k, 300 + k)
    s, c, mu = model
    m = P.PPCAModel(s, c, mu)
    for weights in (w, None):
        got, t = _stats(ctx, P.Dataset(x, weights), m)
        plain = [g for g in t["gemm"] if not g["guarded"] and g["amode"] in (2, 3)]
        print("branch 3", k, t["gemm"])
        assert t["skinny_launches"] == 0 and sorted(g["amode"] for g in plain) == [2, 3], ("branch 3 not reached", t)
        assert all(g["kslices"] >= 3 for g in plain), ("branch 3 not reached", t)
        _assert_stats(got, oracle.stats(x, s, c, mu, weights), d, k, (k, weights is None))


@pytest.mark.parametrize("k,d", [(4, 300), (20, 70), (40, 70)])
def test_guarded_fp64_statistics_product_cut_along_k(P, oracle, ctx, k, d):
    """Branch 3, the fp64 fallback of S: one row x 1e6 trips the chunk's guard at n = 2100 (eight K-slices' worth of rows)."""
    n = 2100
    x, w, (s, c, mu) = _case(oracle, n, d, k, 340 + k)
    x[100] *= 1e6
    got, t = _stats(ctx, P.Dataset(x, w), P.PPCAModel(s, c, mu))
    g2 = [g for g in t["gemm"] if g["amode"] == 2 and g["guarded"]]
    print("branch 3 (guarded)", k, g2)
    assert t["int8"] == 1 and len(g2) == 1 and g2[0]["kslices"] >= 4, ("branch 3 (guarded) not reached", t)
    want = oracle.stats(x, s, c, mu, w)
    _assert_stats(got, want, d, k, (k, "outlier"))
    err = _masked_diag_of_S(got, want, x, 100, d, k)
    print("masked diagonal of S %.2e" % err)
    assert err < 1e-9


def _child(mode, env):
    """tools/split_check.py MODE in a process of its own -> its arrays (the variables it is about are read once per process)"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "out.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "split_check.py"), mode, out], capture_output=True, text=True,
                           env={**os.environ, **env}, timeout=600)
        assert r.returncode == 0 and "split check written" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import split_check
    finally:
        sys.path.pop(0)
    return split_check


def test_fp64_engine_pinned_by_the_environment(P, oracle, ctx):
    """Branch 3 under PPCA_GENERIC_FP64=1 (a child process), k = 4, 20, 40: no int8 launch at all, the statistics product on
    gemm_kernel<2> cut along K; the output passes on the unguarded fp64 Gram."""
    tool = _tool()
    res = _child("fp64", {"PPCA_GENERIC_FP64": "1"})
    for name in tool.CASES["fp64"]:
        x, w, (s, c, mu) = tool.case_data("fp64", name)
        d, k = c.shape
        t = json.loads(str(res[name + "_trace"]))
        g2 = [g for g in t["gemm"] if g["amode"] == 2 and not g["guarded"]]
        print("branch 3 (PPCA_GENERIC_FP64=1)", name, t["gemm"])
        assert t["int8"] == 0 and t["n_i8gemm"] == 0 and g2 and g2[0]["kslices"] >= 4, ("branch 3 (pinned) not reached", t)
        _assert_stats(res[name + "_stats"], oracle.stats(x, s, c, mu, w), d, k, ("fp64", name))
        assert _rel(res[name + "_llks"], oracle.llks(x, s, c, mu)) < TOL_LLK
        want = oracle.llk(x, s, c, mu, w)
        assert abs(float(res[name + "_llk"]) - want) < TOL_LLK * abs(want)
        ti = json.loads(str(res[name + "_trace_infer"]))
        g0 = [g for g in ti["gemm"] if g["amode"] == 0]
        assert ti["em"] == 0 and ti["int8"] == 0 and ti["n_i8gemm"] == 0 and len(g0) == 1 and not g0[0]["guarded"], ti
        st, cv = oracle.infer(x, s, c, mu)
        e1, e2 = _rel(res[name + "_states"], st), _rel(res[name + "_covs"], cv)
        print("fp64", name, "states %.2e covariances %.2e" % (e1, e2))
        assert e1 < TOL_STATE and e2 < TOL_STATE, (name, e1, e2)
        assert _rel(res[name + "_smooth"], oracle.reconstruct(x, s, c, mu, "smooth")) < TOL_RECON
        ex = res[name + "_extrapolate"]
        assert _rel(ex, oracle.reconstruct(x, s, c, mu, "extrapolate")) < TOL_RECON
        assert np.array_equal(ex[np.isfinite(x)], x[np.isfinite(x)]), name
        for what in ("smooth", "extrapolate"):
            assert _rel(res[name + "_diag_" + what], oracle.covariance_diagonal(x, s, c, mu, what)) < TOL_STATE, (name, what)


# ------------------------------------------------------------------ branch 4
@pytest.mark.parametrize("k,d", [(10, 300), (20, 513), (40, 300), (50, 513), (70, 300)])
def test_skinny_products_with_many_slices(P, oracle, ctx, k, d):
    """Branch 4.  skinny_xt_kernel<1..5> (256 threads up to k = 31, 512 beyond) over two or three blocks of dimensions and twelve
    slices of samples of which the last is short; weighted and not."""
    n = 3001
    x, w, (s, c, mu) = _case(oracle, n, d, k, 400 + k)
    m = P.PPCAModel(s, c, mu)
    for weights in (w, None):
        got, t = _stats(ctx, P.Dataset(x, weights), m)
        print("branch 4", k, {a: t[a] for a in ("skinny_launches", "skinny_nt", "skinny_slices", "skinny_gy", "skinny_rps")})
        assert t["skinny_launches"] == 1 and t["skinny_nt"] == (k + 1 + 15) // 16 and t["skinny_gy"] == (d + 255) // 256, ("branch 4 not reached", t)
        assert t["skinny_slices"] >= 8 and n % t["skinny_rps"] != 0 and 0 < n - (t["skinny_slices"] - 1) * t["skinny_rps"] < t["skinny_rps"], t
        _assert_stats(got, oracle.stats(x, s, c, mu, weights), d, k, (k, d, weights is None))


# ------------------------------------------------------------------ branch 5
def _solver_case(P, oracle, ctx, rows, d, k, kinds, nb, min_iters, seed):
    """rows: {grid limit: n}, the first entry also for the output passes"""
    for i, (cap, n) in enumerate(rows.items()):
        _solver_leg(P, oracle, ctx, n, d, k, kinds, nb, cap, min_iters, seed + 50 * i, post=i == 0)


def _solver_leg(P, oracle, ctx, n, d, k, kinds, nb, cap, min_iters, seed, post):
    x, w, model = _case(oracle, n, d, k, seed)
    s, c, mu = model
    m = P.PPCAModel(s, c, mu)

    def check(t, cap, what):
        iters = t["solver_rows"] / (t["solver_grid"] * t["solver_batch"])
        print("branch 5", (k, cap, what), {a: t[a] for a in ("solver", "solver_nb", "solver_grid", "solver_batch", "solver_rows")},
              "iterations per workgroup %.1f" % iters)
        assert t["solver"] in kinds and t["solver_nb"] == nb and t["solver_rows"] == n, ("branch 5: another solver", k, cap, what, t)
        assert iters >= min_iters, ("branch 5 not reached", k, cap, what, iters)

    ctx.set_grid_limit(cap)
    for weights in (w, None):
        got, t = _stats(ctx, P.Dataset(x, weights), m)
        check(t, cap, "em")
        _assert_stats(got, oracle.stats(x, s, c, mu, weights), d, k, (k, cap, weights is None))
    if post:
        _post_against_oracle(P, oracle, ctx, x, w, model, ("solver", k, cap), expect=lambda t, what: check(t, cap, what))


@pytest.mark.parametrize("k", [1, 5, 9, 13, 16])
def test_lane_solver_persistent_loop(P, oracle, ctx, k):
    """Branch 5, one lane per sample (k <= 16; the one-wave-per-SIMD kernel from k = 13): at most 8 blocks of 256 samples per "CU", so
    one workgroup's sweep is 2048 samples per "CU": 20 000 rows on one "CU" (9.8 sweeps) and 33 001 on two (8.06), >= 8 asserted on
    both.  EM and output instantiations."""
    _solver_case(P, oracle, ctx, {1: 20_000, 2: 33_001}, 300, k, (LANE_WIDE,) if k >= 13 else (LANE,), k, 8, 500 + k)


@pytest.mark.parametrize("k", [17, 32, 33, 48, 49, 64])
def test_batched_blocked_solver_persistent_loop(P, oracle, ctx, k):
    """Branch 5, solve4_kernel<2..4> (several samples per wave, diagonal blocks by DPP): >= 50 groups per wave one after the other --
    the inputs of a group are requested half a group ahead, the LDS image is rebuilt in place."""
    _solver_case(P, oracle, ctx, {2: 3001, 1: 3001}, 70, k, (SOLVE4,), (k + 15) // 16, 50, 520 + k)


@pytest.mark.parametrize("k", [65, 80, 81, 96, 97, 112, 113, 128])
def test_mfma_solver_persistent_loop_at_large_state_sizes(P, oracle, ctx, k):
    """Branch 5, solve_mfma_body<5..8> (one sample per wave, the LDS area of a wave re-used by its next sample): >= 50 samples per wave."""
    _solver_case(P, oracle, ctx, {2: 601, 1: 601}, 70, k, (MFMA,), (k + 15) // 16, 50, 560 + k)


# ------------------------------------------------------------------ branches 6 and 8
def test_chunks_beyond_the_capped_grids(P, oracle, ctx):
    """Branches 6 and 8 (a child process under PPCA_GEN_CHUNK=16448): three chunks of more than 16 384 rows, the weights 2^20 larger from
    chunk to chunk -- the scales predicted from the chunk before fail for every column and gen_wdigits_kernel cuts them again with its
    grid capped at 256 row blocks for 257; the scalars reduced over five blocks per chunk and, in the output passes, ADDED to those of the
    chunks before.  Statistics, per-sample and total log-likelihood and the smoothed reconstruction across the chunks.
    With such weights every sum is dominated by its last chunk (the first weighs 2^-40, the second 2^-20 of every block), so the same
    rows run a second time with ordinary weights ("flat": no column is cut again, every chunk weighs the same), and every output pass
    runs across the chunks in this process too (gen_chunk reads the variable per call): per-row outputs know no weights.  Whether a
    column is cut again is decided on the device; the record shows that the re-cut launch was capped, the construction (a scale 2^20
    above the predicted one fails gen_colscale_kernel's acceptance test) that it had columns to cut."""
    tool = _tool()
    res = _child("chunks", {"PPCA_GEN_CHUNK": str(tool.CHUNK)})
    x, w, (s, c, mu) = tool.case_data("chunks", "grow")
    d, k = c.shape
    t = json.loads(str(res["grow_trace"]))
    print("branch 6", {a: t[a] for a in ("chunks", "chunk_rows", "wdigits_first", "wdigits_predicted", "wdigits_y_capped", "scal_blocks_max")})
    assert t["chunks"] == 3 and t["chunk_rows"] > 16384, ("branch 6 not reached", t)
    assert t["wdigits_first"] == 1 and t["wdigits_predicted"] == 2 and t["wdigits_y_capped"] == 2, ("branch 6 not reached", t)
    _assert_stats(res["grow_stats"], oracle.stats(x, s, c, mu, w), d, k, ("chunks",))
    t = json.loads(str(res["grow_trace_llk"]))
    print("branch 8", {a: t[a] for a in ("chunks", "scal_launches", "scal_blocks_max", "scal_accumulated")})
    assert t["em"] == 0 and t["scal_launches"] == 3 and t["scal_accumulated"] == 2 and t["scal_blocks_max"] >= 5, ("branch 8 not reached", t)
    assert _rel(res["grow_llks"], oracle.llks(x, s, c, mu)) < TOL_LLK
    want = oracle.llk(x, s, c, mu, w)
    assert abs(float(res["grow_llk"]) - want) < TOL_LLK * abs(want)
    assert json.loads(str(res["grow_trace_smooth"]))["chunks"] == 3
    assert _rel(res["grow_smooth"], oracle.reconstruct(x, s, c, mu, "smooth")) < TOL_RECON
    x, w, (s, c, mu) = tool.case_data("chunks", "flat")
    t = json.loads(str(res["flat_trace"]))
    assert t["chunks"] == 3 and t["wdigits_predicted"] == 2 and t["wdigits_y_capped"] == 2 and t["scal_launches"] == 3, t
    _assert_stats(res["flat_stats"], oracle.stats(x, s, c, mu, w), d, k, ("chunks", "flat"))
    want = oracle.llk(x, s, c, mu, w)
    assert abs(float(res["flat_llk"]) - want) < TOL_LLK * abs(want)
    assert _rel(res["flat_llks"], oracle.llks(x, s, c, mu)) < TOL_LLK

    def expect(t, what):
        assert t["chunks"] == 3 and t["scal_accumulated"] == 2, ("branch 8 not reached", what, t)

    old = os.environ.get("PPCA_GEN_CHUNK")
    os.environ["PPCA_GEN_CHUNK"] = str(tool.CHUNK)
    try:
        _post_against_oracle(P, oracle, ctx, x, w, (s, c, mu), ("chunks", "flat"), expect=expect)
    finally:
        if old is None:
            del os.environ["PPCA_GEN_CHUNK"]
        else:
            os.environ["PPCA_GEN_CHUNK"] = old


def test_scalar_reduction_with_many_blocks(P, oracle, ctx):
    """Branch 8 in one chunk: 53 001 rows are 13 blocks of scal_reduce_kernel (EM: added to the cleared statistics; output passes: stored)."""
    n, d, k = 53_001, 260, 2
    x, w, (s, c, mu) = _case(oracle, n, d, k, 800)
    m, ds = P.PPCAModel(s, c, mu), P.Dataset(x, w)
    got, t = _stats(ctx, ds, m)
    print("branch 8", {a: t[a] for a in ("chunks", "scal_launches", "scal_blocks_max")})
    assert t["chunks"] == 1 and t["scal_blocks_max"] >= 12, ("branch 8 not reached", t)
    _assert_stats(got, oracle.stats(x, s, c, mu, w), d, k, ("scalars",))

    def expect(t, what):
        assert t["chunks"] == 1 and t["scal_blocks_max"] >= 12, ("branch 8 not reached", what, t)

    _post_against_oracle(P, oracle, ctx, x, w, (s, c, mu), ("scalars",), expect=expect)


# ------------------------------------------------------------------ branch 7
@pytest.mark.parametrize("cap", [16, 2])
def test_reconstruction_with_many_rows_per_block(P, oracle, ctx, cap):
    """Branch 7.  recon2_kernel takes max(16, rows / (8 CUs) + 1) rows per block, at most 256: d = 300 (two blocks along the dimensions),
    n = 5003 on 16 "CUs" and on 2 (more rows per block; a short last block on both); every output pass."""
    n, d, k = 5003, 300, 4
    x, w, model = _case(oracle, n, d, k, 700)
    ctx.set_grid_limit(cap)
    tr = _post_against_oracle(P, oracle, ctx, x, w, model, ("recon", cap))
    for what in ("smooth", "extrapolate", "diag_smooth", "diag_extrapolate"):
        t = tr[what]
        print("branch 7", cap, what, {a: t[a] for a in ("recon_kind", "recon_rpb", "recon_grid_x", "recon_grid_y")})
        assert t["recon_kind"] == 2 and t["recon_rpb"] > 16 and t["recon_grid_y"] == 2, ("branch 7 not reached", what, t)
        assert n % t["recon_rpb"] != 0 and t["recon_grid_x"] == -(-n // t["recon_rpb"])


# ------------------------------------------------------------------ branch 9
def test_int8_gemm_by_pointer_arithmetic(P, oracle, ctx):
    """Branch 9 (child processes): PPCA_I8GEMM_PTR=1 -- the addressing form production takes when an operand reaches 2 GiB -- on three
    shapes that together make the 128-row tile, the 256-row tile, the XCD-aware tile order and a product cut along the samples;
    against the oracle, and bit for bit against the default (buffer) addressing: the same integers summed in the same order."""
    tool = _tool()
    ptr, buf = _child("ptr", {"PPCA_I8GEMM_PTR": "1"}), _child("ptr", {})
    seen = set()
    for name in tool.CASES["ptr"]:
        x, w, (s, c, mu) = tool.case_data("ptr", name)
        d, k = c.shape
        tp, tb = json.loads(str(ptr[name + "_trace"])), json.loads(str(buf[name + "_trace"]))
        print("branch 9", name, tp["i8gemm"])
        assert tp["n_i8gemm"] >= 2 and all(g["buffer"] == 0 for g in tp["i8gemm"]), ("branch 9 not reached", tp)
        assert all(g["buffer"] == 1 for g in tb["i8gemm"]) and [dict(g, buffer=1) for g in tp["i8gemm"]] == tb["i8gemm"]
        for g in tp["i8gemm"]:
            seen |= {("tile", g["tile_rows"]), ("xcd", g["xcd_map"]), ("sliced", g["nsplit"] > 1)}
        _assert_stats(ptr[name + "_stats"], oracle.stats(x, s, c, mu, w), d, k, ("ptr", name))
        assert np.array_equal(ptr[name + "_stats"], buf[name + "_stats"]), name
    assert {("tile", 128), ("tile", 256), ("xcd", 1), ("xcd", 0), ("sliced", True)} <= seen, ("branch 9: a form not reached", seen)


# ------------------------------------------------------------------ retired switches
RETIRED_SWITCHES = {  # every variable the split pipeline once read and no longer does, at its non-default value
    "PPCA_GENERIC_SOLVE": "bc", "PPCA_GENERIC_REG_SOLVE": "1", "PPCA_GENERIC_LDS_SOLVE": "1", "PPCA_GENERIC_LANE_SOLVE": "0",
    "PPCA_SOLVE4": "0", "PPCA_SOLVE_BIG": "1", "PPCA_SOLVE_OCC2": "0", "PPCA_GENERIC_RECON": "naive", "PPCA_GENERIC_PREP": "0",
    "PPCA_GENERIC_SKINNY": "0", "PPCA_GENERIC_BIG_FP64": "1", "PPCA_I8GEMM_TM": "128", "PPCA_I8GEMM_GRAM_TM": "128",
    "PPCA_I8GEMM_S256": "0", "PPCA_I8GEMM_XCD": "0",
}


def test_retired_switches_are_inert(P, oracle, ctx):
    """A child process under every retired switch of the split pipeline at once, on the smallest shapes at which each used to change
    the route: the EM statistics and the smoothed reconstruction against the oracle, and the dispatch record shows the default route --
    d = 300, k = 8: lane solver, the one-pass skinny products, the one pre-solve pass (no gemm_kernel<1>), recon2_kernel;
    d = 70, k = 32, n = 4200: solve4 on two blocks per side, the Gram on 256-row tiles in the XCD-aware order (528 packed columns = 17
    column blocks); d = 1024, k = 4: the statistics product on 256-row tiles; d = k = 70: one sample per wave on the MFMA with five blocks
    per side, the int8 contractions, recon_kernel."""
    tool = _tool()
    res = _child("inert", RETIRED_SWITCHES)
    tr = {}
    for name in tool.CASES["inert"]:
        x, w, (s, c, mu) = tool.case_data("inert", name)
        d, k = c.shape
        tr[name] = t, ts = json.loads(str(res[name + "_trace"])), json.loads(str(res[name + "_trace_smooth"]))
        print("inert", name, {a: t[a] for a in ("solver", "solver_nb", "int8", "skinny_launches")}, t["i8gemm"], t["gemm"], "recon", ts["recon_kind"])
        assert t["valid"] == 1 and t["em"] == 1 and (t["d"], t["k"], t["n"]) == (d, k, len(x)) and ts["em"] == 0, (name, t, ts)
        _assert_stats(res[name + "_stats"], oracle.stats(x, s, c, mu, w), d, k, ("inert", name))
        err = _rel(res[name + "_smooth"], oracle.reconstruct(x, s, c, mu, "smooth"))
        print("inert", name, "smooth %.2e" % err)
        assert err < TOL_RECON, (name, err)
    t, ts = tr["lane"]
    assert t["solver"] == LANE and ts["solver"] == LANE, t
    assert t["skinny_launches"] == 1 and not [g for g in t["gemm"] if g["amode"] == 1] and ts["recon_kind"] == 2, (t, ts)
    t, ts = tr["solve4"]
    gram = [g for g in t["i8gemm"] if g["role"] == 0]
    assert t["solver"] == SOLVE4 and t["solver_nb"] == 2 and ts["solver"] == SOLVE4, t
    assert len(gram) == 1 and gram[0]["tile_rows"] == 256 and gram[0]["xcd_map"] == 1, t
    t, ts = tr["tall"]
    stat = [g for g in t["i8gemm"] if g["role"] == 1]
    assert len(stat) == 1 and stat[0]["tile_rows"] == 256, t
    t, ts = tr["mfma"]
    assert t["solver"] == MFMA and t["solver_nb"] == 5 and t["int8"] == 1 and ts["solver"] == MFMA and ts["recon_kind"] == 1, (t, ts)


# ------------------------------------------------------------------ the output passes of k = 11..16 at d <= 256
@pytest.mark.parametrize("k,d", [(11, 256), (12, 64), (13, 200), (14, 255), (15, 100), (16, 200)])
def test_output_passes_of_the_two_kernel_shapes(P, oracle, ctx, k, d):
    """The EM pass of 11 <= k <= 16, d <= 256 is the two-kernel pass (ppca_em16.hip); every OTHER pass of these shapes stays on the split
    pipeline -- launch_solve_lane<11..16, false>, from k = 13 the one-wave-per-SIMD kernel -- here 33 001 rows on two "CUs" (8.06 sweeps of 2048 samples each, >= 8 asserted)."""
    n = 33_001
    x, w, model = _case(oracle, n, d, k, 900 + k)
    ctx.set_grid_limit(2)
    s, c, mu = model
    _, t = _stats(ctx, P.Dataset(x, w), P.PPCAModel(s, c, mu), fused16=1)
    assert t["n_i8gemm"] == 0 and t["solver_launches"] == 0, t

    def expect(t, what):
        assert t["solver"] == (LANE_WIDE if k >= 13 else LANE) and t["solver_nb"] == k, ("another solver", k, what, t)
        assert t["solver_rows"] / (t["solver_grid"] * t["solver_batch"]) >= 8, ("persistent loop not reached", k, what, t)

    _post_against_oracle(P, oracle, ctx, x, w, model, ("k11..16", k), expect=expect)

