"""PPCAModel.recommend on the GPU: the n best columns per row of a SparseDataset.

1. exact, against the library's own predict at all N d positions and the restated rule of tests/topn_cases.py (the scores are predict's
   bit for bit, so columns and scores must be equal, not close);  2. against the oracle's smooth, by set and tolerance (the oracle's
   scores differ from the library's in the last bits, and every case has rows whose leading scores lie closer than that);  3. ties;
4. the seams of the 64-column tile and of rows with d, d - 1, d - n, d - n + 1, 0 and 1 entries;  5. bit-identical results under any
grid limit and block_rows, with and without the column split;  6. a shape the dense layout cannot hold.

Tolerance where one is needed: the project's GPU parity bound, 1e-5, relative to 1 + |value| (tests/test_gpu_sparse.py)."""
import functools

import numpy as np
import pytest

import sparse_cases as SC
import state_size_cases as S
import topn_cases as TC

pytestmark = pytest.mark.gpu

TOL = 1e-5
KAPPAS = (0.0, 1.5, -1.0)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


@functools.lru_cache(maxsize=None)
def _case(n, d, k):
    x, w, model = SC.case(n, d, k)
    for a in (x, w) + tuple(model[1:]):
        a.setflags(write=False)
    return x, w, model


def _predict_all(model, sp, n, d):
    mean, var = model.predict(sp, TC.all_positions(n, d))
    return mean.reshape(n, d), var.reshape(n, d)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


def _check_exact(model, sp, x, ns, label):
    """recommend against topn_reference on predict's values: every kappa, n, exclude_observed and candidate list."""
    n, d = x.shape
    obs = np.isfinite(x)
    mean, var = _predict_all(model, sp, n, d)
    assert np.all(var > 0)
    for kappa in KAPPAS:
        score = TC.score(mean, var, kappa)
        for cand in (None, np.arange(0, d, 3), np.zeros(0, dtype=np.int64)):
            for exclude in (True, False):
                for n_top in ns:
                    got = model.recommend(sp, n_top, kappa=kappa, exclude_observed=exclude, candidates=cand)
                    want = TC.topn_reference(score, obs if exclude else None, n_top, cand)
                    what = (label, kappa, None if cand is None else cand.size, exclude, n_top)
                    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[0].shape == got[1].shape == (n, n_top), what
                    assert np.array_equal(got[0], want[0]), what
                    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), what  # (TC.fma: bit-identical at every kappa)


# ------------------------------------------------------------------ 1. exact, against predict
EXACT = [(64, 9, 3), (257, 300, 1), (150, 300, 11), (64, 9, 0), (120, 200, 16)]


@pytest.mark.parametrize("n,d,k", EXACT, ids=["%dx%dx%d" % s for s in EXACT])
def test_exact_against_predict(P, n, d, k):
    x, w, (s, c, mu) = _case(n, d, k)
    sp = P.SparseDataset.from_dense(x, w)
    _check_exact(P.PPCAModel(s, c, mu), sp, x, (1, 10, 64), "%dx%dx%d" % (n, d, k))


@pytest.mark.parametrize("k", range(17))
def test_exact_state_size_sweep(P, k):
    """Every instantiation of the top-n kernel against predict, which tests/test_gpu_sparse.py holds to the oracle on the same case."""
    x, w, (s, c, mu) = _case(*S.SPARSE, k)
    sp = P.SparseDataset.from_dense(x, w)
    _check_exact(P.PPCAModel(s, c, mu), sp, x, (10,), "%dx%dx%d" % (S.SPARSE + (k,)))


# ------------------------------------------------------------------ 2. against the oracle
def _check_against(cols, scores, want, obs, n_top, label):
    """The five per-row properties of a returned list against reference scores `want` (N, d); candidates: the unobserved columns."""
    n, d = want.shape
    worst_score, worst_cut = 0.0, -np.inf
    for i in range(n):
        candidates = np.flatnonzero(~obs[i])
        ni = min(n_top, candidates.size)
        ci, si = cols[i], scores[i]
        assert np.all(ci[:ni] >= 0) and np.all(ci[ni:] == -1) and np.all(np.isfinite(si[:ni])) and np.all(np.isnan(si[ni:])), (label, i)
        assert np.unique(ci[:ni]).size == ni and not obs[i, ci[:ni]].any(), (label, i)
        step = np.diff(si[:ni])
        assert np.all(step <= 0) and np.all(np.diff(ci[:ni])[step == 0] > 0), (label, i)
        if ni == 0:
            continue
        worst_score = max(worst_score, _rel(si[:ni], want[i, ci[:ni]]))
        cut = np.partition(want[i, candidates], candidates.size - ni)[candidates.size - ni]  # the ni-th largest
        worst_cut = max(worst_cut, float((cut - want[i, ci[:ni]].min()) / (1.0 + abs(cut))))
    print("%s: scores %.1e (bound %g), cut-off missed by %.1e (bound %g)" % (label, worst_score, TOL, max(worst_cut, 0.0), 2 * TOL))
    assert worst_score <= TOL and worst_cut <= 2 * TOL, label


ORACLE = [((64, 9, 3), (10,)), ((300, 2000, 10), (10,)), ((200, 1500, 16), (10, 64)), ((40, 70000, 3), (10, 64))]


@pytest.mark.parametrize("shape,ns", ORACLE, ids=["%dx%dx%d" % s for s, _ in ORACLE])
def test_against_oracle(P, oracle, shape, ns):
    n, d, k = shape
    x, w, (s, c, mu) = _case(n, d, k)
    obs = np.isfinite(x)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(s, c, mu)
    smooth = oracle.reconstruct(x, s, c, mu, "smooth")
    for n_top in ns:
        cols, scores = model.recommend(sp, n_top)
        _check_against(cols, scores, smooth, obs, n_top, "oracle %dx%dx%d n=%d" % (n, d, k, n_top))
    if shape == (300, 2000, 10):
        _, cov = oracle.infer(x, s, c, mu)
        var = np.einsum("ja,iab,jb->ij", c, cov, c) + s * s
        cols, scores = model.recommend(sp, 10, kappa=1.5)
        _check_against(cols, scores, smooth + 1.5 * np.sqrt(var), obs, 10, "oracle %dx%dx%d kappa=1.5" % shape)


# ------------------------------------------------------------------ 3. ties
def test_ties(P):
    x, w, (s, c, mu), same = TC.tie_case()
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(s, c, mu)
    mean, var = _predict_all(model, sp, *x.shape)
    assert all(np.array_equal(mean[:, same[0]], mean[:, j]) and np.array_equal(var[:, same[0]], var[:, j]) for j in same)
    ctx = sp._ctx
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            for kappa in (0.0, 1.5):
                want = TC.topn_reference(TC.score(mean, var, kappa), np.isfinite(x), 10)
                got = model.recommend(sp, 10, kappa=kappa)
                assert np.array_equal(got[0][:, :4], np.tile(same, (32, 1))), (limit, kappa)
                assert all(np.array_equal(got[1][:, 0], got[1][:, p]) for p in range(4)), (limit, kappa)
                assert _same(got, want), (limit, kappa)
                assert np.array_equal(model.recommend(sp, 2, kappa=kappa)[0], np.tile(same[:2], (32, 1))), (limit, kappa)
    finally:
        ctx.set_grid_limit(0)


def test_constant_scores_give_the_first_candidates(P):
    """State size 0 and one mean everywhere: every candidate ties, the answer is each row's first n candidate columns."""
    x, w, _ = _case(257, 300, 1)
    n, d = x.shape
    obs = np.isfinite(x)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(0.7, np.zeros((d, 0)), np.full(d, 1.25))
    for cand in (None, np.arange(1, d, 7)):
        cols, scores = model.recommend(sp, 10, candidates=cand)
        pool = np.arange(d) if cand is None else cand
        for i in range(n):
            first = pool[~obs[i, pool]][:10]
            assert np.array_equal(cols[i, :first.size], first) and np.all(cols[i, first.size:] == -1), i
            assert np.all(scores[i, :first.size] == 1.25) and np.all(np.isnan(scores[i, first.size:])), i
    cols, _ = model.recommend(sp, 64, exclude_observed=False)
    assert np.array_equal(cols, np.tile(np.arange(64, dtype=np.int32), (n, 1)))


# ------------------------------------------------------------------ 4. seams
@pytest.mark.parametrize("d", [1, 63, 64, 65, 129])
def test_seams(P, d):
    x, (s, c, mu) = TC.seam_case(d)
    lengths = np.isfinite(x).sum(axis=1)
    assert tuple(lengths[:6]) == tuple(min(max(m, 0), d) for m in (d, d - 1, d - 5, d - 4, 0, 1))
    sp = P.SparseDataset.from_dense(x)
    _check_exact(P.PPCAModel(s, c, mu), sp, x, (5, 64), "seams d=%d" % d)


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("n,d,k", [(40, 70000, 3), (300, 2000, 10)], ids=["40x70000x3", "300x2000x10"])
def test_determinism(P, n, d, k):
    x, w, (s, c, mu) = _case(n, d, k)
    model = P.PPCAModel(s, c, mu)
    sp = P.SparseDataset.from_dense(x, w)
    tiled = [P.SparseDataset.from_dense(x, w, block_rows=br) for br in (64, 16)]
    calls = [dict(n=10), dict(n=64, kappa=1.0), dict(n=10, kappa=-1.0, exclude_observed=False, candidates=np.arange(2, d, 5))]
    ref = [model.recommend(sp, **kw) for kw in calls]
    ctx = sp._ctx
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            for ds in [sp] + tiled:
                for kw, r in zip(calls, ref):
                    assert _same(model.recommend(ds, **kw), r), (limit, ds._block_rows, sorted(kw))
    finally:
        ctx.set_grid_limit(0)
    # a row's list depends on the row alone: the second half, without weights
    half = P.SparseDataset.from_dense(x[n // 2:])
    assert _same(model.recommend(half, 10), (ref[0][0][n // 2:], ref[0][1][n // 2:]))


# ------------------------------------------------------------------ 6. capacity
def test_capacity(P):
    """N = 100 000 x d = 500 000 with 20 entries per row (the data of tests/test_gpu_sparse.py::test_capacity): 400 GB as a dense array."""
    n, d, k, per, n_top = 100_000, 500_000, 4, 20, 10
    rng = np.random.default_rng(2024)
    c_true, mu_true = rng.standard_normal((d, k)), rng.standard_normal(d)
    hot = 2000
    cols = np.where(rng.random((n, per)) < 0.9, rng.integers(0, hot, (n, per)), rng.integers(0, d, (n, per)))
    cols.sort(axis=1)
    keep = np.concatenate([np.ones((n, 1), dtype=bool), np.diff(cols, axis=1) > 0], axis=1)  # no duplicate within a row
    z = rng.standard_normal((n, k))
    vals = np.einsum("nk,npk->np", z, c_true[cols]) + mu_true[cols] + 0.5 * rng.standard_normal((n, per))
    indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    sp = P.SparseDataset(indptr, cols[keep].astype(np.int32), vals[keep], d)
    model = P.PPCAModel(0.5, c_true, mu_true)

    got_cols, got_scores = model.recommend(sp, n_top)
    assert got_cols.shape == got_scores.shape == (n, n_top) and got_cols.dtype == np.int32
    assert got_cols.min() >= 0 and got_cols.max() < d and np.all(np.isfinite(got_scores))
    assert np.all(np.diff(got_scores, axis=1) <= 0)
    hit = (got_cols[:, :, None] == cols[:, None, :]) & keep[:, None, :]
    assert not hit.any()  # no observed column is returned

    sample = np.sort(rng.choice(n, size=200, replace=False))
    for lo in range(0, sample.size, 25):
        rows = sample[lo:lo + 25]
        q_indptr = np.zeros(n + 1, dtype=np.int64)
        q_indptr[rows + 1] = d
        mean, _ = model.predict(sp, (np.cumsum(q_indptr), np.tile(np.arange(d, dtype=np.int32), rows.size)))
        mean = mean.reshape(rows.size, d)
        for t, i in enumerate(rows):
            mean[t, cols[i][keep[i]]] = -np.inf  # the row's own columns leave the candidate set
            lead = np.flatnonzero(mean[t] >= np.partition(mean[t], d - n_top)[d - n_top])  # every column that can be among the n best
            want = TC.topn_reference(mean[t:t + 1], None, n_top, lead)
            assert _same((got_cols[i:i + 1], got_scores[i:i + 1]), want), i
