"""PPCAMix.recommend on the GPU: the n best columns per row of a SparseDataset under a mixture.

1. exact, against the mixture's own predict at all N d positions and the rule of tests/topn_cases.py (the scores are predict's bit for
   bit -- test_gpu_sparse_mix.py holds predict to the oracle -- so columns and scores must be equal, not close);  2. every state size;
3. components of different state sizes, more components than one group of the row pass, a component of weight 0;  4. one component
against PPCAModel.recommend;  5. against the oracle, by the five per-row properties of tests/mix_topn_cases.py;  6. ties;  7. the seams
of the 64-column tile and of the row lengths;  8. bit-identical results under any grid limit and block_rows, with and without the
column split;  9. the refusals of the C entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

import mix_topn_cases as XC
import sparse_mix_cases as MC
import topn_cases as TC

pytestmark = pytest.mark.gpu

INVALID = -1
KAPPAS = XC.KAPPAS


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@functools.lru_cache(maxsize=None)
def _case(n, d, k, nm):
    x, w, (s, c, mu), lw, _ = MC.mix_case(n, d, k, nm)
    for a in (x, w, s, c, mu, lw):
        a.setflags(write=False)
    return x, w, (s, c, mu), lw


def _mix(P, model, lw, sizes=None):
    s, c, mu = model
    sizes = [c.shape[2]] * len(s) if sizes is None else sizes
    return P.PPCAMix([P.PPCAModel(s[i], np.ascontiguousarray(c[i][:, :sizes[i]]), mu[i]) for i in range(len(s))], lw)


def _predict_all(model, sp, n, d):
    mean, var = model.predict(sp, TC.all_positions(n, d))
    return mean.reshape(n, d), var.reshape(n, d)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


def _check_exact(mix, sp, x, ns, label, cands=None, kappas=KAPPAS):
    """recommend against topn_reference on predict's values: every kappa, n, exclude_observed and candidate list."""
    n, d = x.shape
    obs = np.isfinite(x)
    mean, var = _predict_all(mix, sp, n, d)
    assert np.all(var > 0)
    cands = (None, np.arange(0, d, 3), np.zeros(0, dtype=np.int64)) if cands is None else cands
    for kappa in kappas:
        score = TC.score(mean, var, kappa)
        for cand in cands:
            for exclude in (True, False):
                for n_top in ns:
                    got = mix.recommend(sp, n_top, kappa=kappa, exclude_observed=exclude, candidates=cand)
                    want = TC.topn_reference(score, obs if exclude else None, n_top, cand)
                    what = (label, kappa, None if cand is None else cand.size, exclude, n_top)
                    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == got[1].shape == (n, n_top), what
                    assert np.array_equal(got[0], want[0]), what
                    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), what


# ------------------------------------------------------------------ 1. exact, against predict
@pytest.mark.parametrize("n,d,k,nm", XC.EXACT, ids=["%dx%dx%d-nm%d" % s for s in XC.EXACT])
def test_exact_against_predict(P, n, d, k, nm):
    x, w, model, lw = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    _check_exact(_mix(P, model, lw), sp, x, (1, 10, 64), "%dx%dx%d nm %d" % (n, d, k, nm))


# ------------------------------------------------------------------ 2. every state size
@pytest.mark.parametrize("n,d,k,nm", XC.SIZES, ids=["k%d" % s[2] for s in XC.SIZES])
def test_exact_state_size_sweep(P, n, d, k, nm):
    """Every instantiation of the mixture's top-n kernel (both tile heights: kappa = 0 and kappa != 0) against predict."""
    x, w, model, lw = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw)
    assert mix.state_sizes == [k] * nm
    _check_exact(mix, sp, x, (10,), "%dx%dx%d nm %d" % (n, d, k, nm), cands=(None,))


# ------------------------------------------------------------------ 3. mixed state sizes, many components, a weight of 0
@pytest.mark.parametrize("shape,sizes", XC.MIXED, ids=["sizes-" + "-".join(map(str, s)) for _, s in XC.MIXED])
def test_exact_mixed_state_sizes(P, shape, sizes):
    x, w, model, lw = _case(*shape)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw, sizes)
    assert mix.state_sizes == list(sizes)
    _check_exact(mix, sp, x, (10,), "mixed sizes %s" % (sizes,))


def test_exact_one_component_past_a_group_of_the_row_pass(P):
    x, w, model, lw = _case(*XC.MANY)
    sp = P.SparseDataset.from_dense(x, w)
    _check_exact(_mix(P, model, lw), sp, x, (10,), "nm 17")


@pytest.mark.parametrize("dead", [0, 1])
def test_exact_with_a_component_of_weight_zero(P, dead):
    x, w, model, lw = _case(64, 9, 3, 3)
    lw = lw.copy()
    lw[dead] = -np.inf
    sp = P.SparseDataset.from_dense(x, w)
    with np.errstate(divide="ignore"):
        mix = _mix(P, model, lw)
    assert mix.weights[dead] == 0.0 and np.exp(mix.infer_cluster(sp))[:, dead].max() == 0.0
    _check_exact(mix, sp, x, (10,), "component %d of weight 0" % dead)


# ------------------------------------------------------------------ 4. one component
@pytest.mark.parametrize("n,d,k,nm", XC.ONE, ids=["%dx%dx%d" % s[:3] for s in XC.ONE])
def test_one_component_is_the_models_recommend(P, n, d, k, nm):
    x, w, (s, c, mu), _ = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(s[0], c[0], mu[0])
    mix = P.PPCAMix([model], [0.3])
    for kappa in KAPPAS:
        for exclude in (True, False):
            for n_top in (10, 64):
                kw = dict(kappa=kappa, exclude_observed=exclude)
                assert _same(mix.recommend(sp, n_top, **kw), model.recommend(sp, n_top, **kw)), (kappa, exclude, n_top)


# ------------------------------------------------------------------ 5. against the oracle
@pytest.mark.parametrize("n,d,k,nm", XC.ORACLE, ids=["%dx%dx%d-nm%d" % s for s in XC.ORACLE])
def test_against_oracle(P, oracle, n, d, k, nm):
    x, w, (s, c, mu), lw = _case(n, d, k, nm)
    obs = np.isfinite(x)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, (s, c, mu), lw)
    ref = oracle.mix_inferred(x, s, c, mu, lw)
    ucb = ref["smooth"] + 1.5 * np.sqrt(ref["smooth_covariance_diagonal"])
    for n_top in (10, 64):
        cols, scores = mix.recommend(sp, n_top)
        XC.check_against(cols, scores, ref["smooth"], obs, n_top, "oracle %dx%dx%d nm %d n=%d" % (n, d, k, nm, n_top))
        cols, scores = mix.recommend(sp, n_top, kappa=1.5)
        XC.check_against(cols, scores, ucb, obs, n_top, "oracle %dx%dx%d nm %d n=%d kappa=1.5" % (n, d, k, nm, n_top))


# ------------------------------------------------------------------ 6. ties
def test_ties(P):
    x, w, model, lw, same = XC.tie_case()
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw)
    mean, var = _predict_all(mix, sp, *x.shape)
    assert all(np.array_equal(mean[:, same[0]], mean[:, j]) and np.array_equal(var[:, same[0]], var[:, j]) for j in same)
    ctx = sp._ctx
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            for kappa in (0.0, 1.5):
                want = TC.topn_reference(TC.score(mean, var, kappa), np.isfinite(x), 10)
                got = mix.recommend(sp, 10, kappa=kappa)
                assert np.array_equal(got[0][:, :4], np.tile(same, (32, 1))), (limit, kappa)
                assert all(np.array_equal(got[1][:, 0], got[1][:, p]) for p in range(4)), (limit, kappa)
                assert _same(got, want), (limit, kappa)
                assert np.array_equal(mix.recommend(sp, 2, kappa=kappa)[0], np.tile(same[:2], (32, 1))), (limit, kappa)
    finally:
        ctx.set_grid_limit(0)


# ------------------------------------------------------------------ 7. seams
@pytest.mark.parametrize("d", XC.SEAM_DS)
def test_seams(P, d):
    x, w, model, lw, _ = XC.seam_case(d)
    assert tuple(np.isfinite(x).sum(axis=1)[:6]) == XC.seam_lengths(d)
    sp = P.SparseDataset.from_dense(x)
    _check_exact(_mix(P, model, lw), sp, x, (5, 64), "seams d=%d" % d)


# ------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("n,d,k,nm", XC.DETERMINISM, ids=["%dx%dx%d-nm%d" % s for s in XC.DETERMINISM])
def test_determinism(P, n, d, k, nm):
    x, w, model, lw = _case(n, d, k, nm)
    mix = _mix(P, model, lw)
    sp = P.SparseDataset.from_dense(x, w)
    tiled = [P.SparseDataset.from_dense(x, w, block_rows=br) for br in (64, 16)]
    calls = [dict(n=10), dict(n=64, kappa=1.0), dict(n=10, kappa=-1.0, exclude_observed=False, candidates=np.arange(2, d, 5))]
    ref = [mix.recommend(sp, **kw) for kw in calls]
    assert all(_same(mix.recommend(sp, **kw), r) for kw, r in zip(calls, ref))  # two consecutive calls
    ctx = sp._ctx
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            for ds in [sp] + tiled:
                for kw, r in zip(calls, ref):
                    assert _same(mix.recommend(ds, **kw), r), (limit, ds._block_rows, sorted(kw))
    finally:
        ctx.set_grid_limit(0)
    # a row's list depends on the row alone: the second half, without weights
    half = P.SparseDataset.from_dense(x[n // 2:])
    assert _same(mix.recommend(half, 10), (ref[0][0][n // 2:], ref[0][1][n // 2:]))


# ------------------------------------------------------------------ 9. errors at the ABI
def test_the_entry_point_refuses_before_it_writes(P, hiplib):
    from ppca_rs_amd._lib import ptr

    x, w, model, lw = _case(64, 9, 3, 2)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw)
    ctx = sp._ctx
    devs, arr = mix._handles(ctx)
    n, n_top = len(sp), 3
    cols, scores = np.full((n, n_top), 7, dtype=np.int32), np.full((n, n_top), 7.0)
    lwp, unsorted = ptr(mix._lw), np.array([0, 4, 2], dtype=np.int32)

    def call(nm=2, n_top=n_top, kappa=0.0, cand=None, n_cand=0, out_c=cols, out_s=scores):
        return hiplib.ppca_mix_topn_sparse(ctx.handle, sp._sh, arr, lwp, nm, n_top, kappa, 1, ptr(cand), n_cand, ptr(out_c), ptr(out_s))

    bad = {"n_models = 0": dict(nm=0), "null columns": dict(out_c=None), "null scores": dict(out_s=None), "n_top = 0": dict(n_top=0),
           "n_top = 65": dict(n_top=65), "kappa NaN": dict(kappa=float("nan")), "kappa inf": dict(kappa=float("inf")),
           "unsorted candidates": dict(cand=unsorted, n_cand=3), "too many candidates": dict(cand=unsorted, n_cand=10)}
    for what, kw in bad.items():
        assert call(**kw) == INVALID, what
        assert (cols == 7).all() and (scores == 7.0).all(), what
    assert call() == 0 and _same((cols, scores), mix.recommend(sp, n_top))
