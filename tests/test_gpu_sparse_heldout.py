"""Held-out scoring of row-compressed data on the GPU: PPCAModel.heldout_score on two SparseDatasets against the
numpy restatement (tests/heldout_restatement.py) and against the library's dense path; the seams of the tiling; what the pass promises
exactly (per-row scores that depend on the row alone, column sums that do not depend on the grid); edge datasets and errors; the host
split against the device split of Dataset.holdout; row shards; and one end-to-end selection of the state size.

Bounds.  TOL = the project's GPU parity tolerance, 1e-5, against the restatement fed the ORACLE's posteriors, with the measures of
tests/test_gpu_heldout.py::_errors (per row relative to 1 + |value|, sums relative to the sum of their terms' magnitudes).  TOL_OWN =
1e-10 (TOL_OWN of the dense test) where both sides use the device's own posteriors: against the restatement fed `infer` of the sparse
train part, and against the dense path.  Every parity check prints its worst error before asserting."""
import ctypes as C
import functools

import numpy as np
import pytest

import heldout_restatement as H
import sparse_cases as SC
import state_size_cases as S
from test_gpu_heldout import _counts_match, _errors, _rel_rows, _rel_sums

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_OWN = 1e-10
INVALID, UNSUPPORTED = -1, -3
SHAPES = [(1, 1, 1), (64, 9, 3), (257, 300, 1), (300, 2000, 10), (200, 1500, 16), (40, 70000, 3), (100, 20, 0)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
QS = ("count", "llk", "se", "z2")


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(n, d, k):
    """x, weights, scoring model of sparse_cases.case and the dense split at 0.3.  Shared and read-only."""
    x, w, (s, c, mu) = SC.case(n, d, k)
    train, held, counts = H.holdout(x, 0.3, 50 + d)
    _freeze(x, w, c, mu, train, held)
    return x, w, (s, c, mu), train, held, counts


@functools.lru_cache(maxsize=None)
def _want(oracle, n, d, k):
    """The restatement's result with the oracle's posteriors of the dense train part (k = 0: the restatement's own)."""
    _, w, (s, c, mu), train, held, _ = _case(n, d, k)
    post = oracle.infer(train, s, c, mu) if k > 0 else H.posteriors(train, s, c, mu)
    res = H.score(train, held, s, c, mu, w=w, post=post)
    _freeze(*[v for v in res.values() if isinstance(v, np.ndarray)])
    return res


def _cols(sc):
    return np.stack([sc.columns[q] for q in QS])


def _same_bits(a, b):
    return np.array_equal(a.llks, b.llks) and np.array_equal(_cols(a), _cols(b)) and (a.n_entries, a.n_rows) == (b.n_entries, b.n_rows)


def _cols_close(sc, base, bound=1e-12):
    """column sums relative to their own magnitude (the measure of test_gpu_heldout.py::test_score_grid_chunks_and_slices)"""
    got, want = _cols(sc), _cols(base)
    err = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
    print("   column sums: %.1e (bound %g)" % (err, bound))
    assert err <= bound


def _show(label, errs, bound):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % bound)


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("n,d,k", SHAPES, ids=IDS)
def test_score_matches_the_restatement(P, oracle, n, d, k):
    _check_score(P, oracle, n, d, k)


@pytest.mark.parametrize("k", range(17))
def test_score_state_size_sweep(P, oracle, k):
    """Every instantiation of the held-out row and column kernels, on the shape whose train rows fall in all three length bins at every
    k (tests/test_state_sizes_host.py)."""
    _check_score(P, oracle, *S.SPARSE, k)


def _check_score(P, oracle, n, d, k):
    x, w, (s, c, mu), train, held, counts = _case(n, d, k)
    res = _want(oracle, n, d, k)
    tsp, hsp, m = P.SparseDataset.from_dense(train, w), P.SparseDataset.from_dense(held), P.PPCAModel(s, c, mu)
    assert (tsp.nnz, hsp.nnz) == counts
    sc = m.heldout_score(tsp, hsp)
    errs = _errors(sc, res)
    _show("sparse score %dx%dx%d vs oracle posteriors:" % (n, d, k), errs, TOL)
    assert _counts_match(sc, res) and sc.n_entries == hsp.nnz and np.all(np.isfinite(sc.llks))
    assert max(errs.values()) <= TOL, errs
    assert np.all(sc.llks[~np.isfinite(held).any(axis=1)] == 0.0)
    if k > 0:  # fed the device's own posteriors of the sparse train part
        inf = m.infer(tsp)
        own = _errors(sc, H.score(train, held, s, c, mu, w=w, post=(inf._states, inf._covs)))
        _show("sparse score %dx%dx%d vs own posteriors:" % (n, d, k), own, TOL_OWN)
        assert max(own.values()) <= TOL_OWN, own
    assert _same_bits(m.heldout_score(tsp, hsp), sc)  # two runs: the same bits


# ------------------------------------------------------------------ 2. against the dense path
@pytest.mark.parametrize("n,d,k", [s_ for s_ in SHAPES if s_[1] <= 2000], ids=[i for s_, i in zip(SHAPES, IDS) if s_[1] <= 2000])
def test_score_matches_the_dense_path(P, oracle, n, d, k):
    x, w, (s, c, mu), train, held, _ = _case(n, d, k)
    res = _want(oracle, n, d, k)
    m = P.PPCAModel(s, c, mu)
    sp = m.heldout_score(P.SparseDataset.from_dense(train, w), P.SparseDataset.from_dense(held))
    de = m.heldout_score(P.Dataset(train, w), P.Dataset(held))
    scale = np.where(res["col_abs"] > 0, res["col_abs"], 1.0)
    errs = dict(rows=_rel_rows(sp.llks, de.llks), cols=_rel_sums(_cols(sp), _cols(de), scale))
    _show("sparse vs dense %dx%dx%d:" % (n, d, k), errs, TOL_OWN)
    assert max(errs.values()) <= TOL_OWN, errs
    assert (sp.n_entries, sp.n_rows) == (de.n_entries, de.n_rows)


# ------------------------------------------------------------------ 3. seams
SEAM = (300, 300, 4)
SEAM_HELD_ROWS = (0, 1, 15, 16, 17, 63, 64, 65, 300)
SEAM_HELD_COLS = (0, 1, 7, 8, 9, 17)


@functools.lru_cache(maxsize=None)
def _seam_case():
    """Patterns written out, not drawn; block_rows = 64 cuts the rows into blocks 0 .. 4.
    Held rows 0-8 (block 0) of exactly 0, 1, 15, 16, 17, 63, 64, 65 and d entries, the last over an empty train row (the prior
    predictive of a whole row); block 1 (rows 64-127) without a held entry; block 2 (rows 128-191) without a train entry; in block 3
    (rows 192-255) the held columns 20-25 have 0, 1, 7, 8, 9 and 17 entries (segment = 8: no item, short items, a full one, runs with a
    remainder) -- counted within the block, the unit the work items are cut by: the full row 8 adds its one entry to every column of
    block 0."""
    n, d, k = SEAM
    i, j = np.arange(n)[:, None], np.arange(d)[None, :]
    tobs = (i * 31 + j * 17) % 11 == 0
    hobs = ((i * 13 + j * 7) % 23 == 1) & ~tobs
    hobs[:, 20:26] = False
    hobs[:9] = False
    for r, m in enumerate(SEAM_HELD_ROWS[:8]):
        hobs[r, 30:30 + m] = True
    hobs[8] = True
    hobs[64:128] = False
    tobs[128:192] = False
    for col, cnt in zip(range(20, 26), SEAM_HELD_COLS):
        hobs[192:192 + cnt, col] = True
    tobs &= ~hobs
    rng = np.random.default_rng(3)
    model = SC.true_model(d, k, rng)
    x = SC.sample(tobs | hobs, model, rng)
    w = 0.5 + rng.random(n)
    w[n // 2] = 0.0
    train, held = np.where(tobs, x, np.nan), np.where(hobs, x, np.nan)
    s, c, mu = SC.scoring_model(model, rng)
    _freeze(train, held, w, c, mu)
    return train, held, w, (s, c, mu)


def test_seams(P, oracle):
    n, d, k = SEAM
    train, held, w, (s, c, mu) = _seam_case()
    hfin, tfin = np.isfinite(held), np.isfinite(train)
    assert tuple(hfin.sum(axis=1)[:9]) == SEAM_HELD_ROWS and not tfin[8].any()
    assert not hfin[64:128].any() and tfin[64:128].any() and not tfin[128:192].any() and hfin[128:192].any()
    assert tuple(hfin[192:256].sum(axis=0)[20:26]) == SEAM_HELD_COLS and not (hfin & tfin).any()
    m = P.PPCAModel(s, c, mu)
    res = H.score(train, held, s, c, mu, w=w, post=oracle.infer(train, s, c, mu))
    base = m.heldout_score(P.SparseDataset.from_dense(train, w), P.SparseDataset.from_dense(held))
    for br, seg in ((64, 8), (64, None), (None, 8), (7, 3)):
        kw = dict(block_rows=br, segment=seg)
        sc = m.heldout_score(P.SparseDataset.from_dense(train, w, **kw), P.SparseDataset.from_dense(held, **kw))
        errs = _errors(sc, res)
        _show("seams block_rows=%s segment=%s:" % (br, seg), errs, TOL)
        assert _counts_match(sc, res) and max(errs.values()) <= TOL, errs
        assert np.array_equal(sc.llks, base.llks), "per_row must not depend on the tiling"
        _cols_close(sc, base)
    # the prior predictive of the full held row over its empty train row
    v = s * s + (c * c).sum(axis=1)
    want = float((-0.5 * (H.LN_2PI + np.log(v) + (held[8] - mu) ** 2 / v)).sum())
    assert abs(base.llks[8] - want) <= TOL_OWN * (1.0 + abs(want))


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("n,d,k", [(300, 2000, 10), (200, 1500, 16)])
def test_determinism(P, n, d, k):
    _, w, (s, c, mu), train, held, _ = _case(n, d, k)
    m = P.PPCAModel(s, c, mu)
    sets = {br: (P.SparseDataset.from_dense(train, w, block_rows=br, segment=8), P.SparseDataset.from_dense(held, block_rows=br, segment=8))
            for br in (64, n)}
    ref = {br: m.heldout_score(*pair) for br, pair in sets.items()}
    assert np.array_equal(ref[64].llks, ref[n].llks)
    _cols_close(ref[64], ref[n])
    ctx = sets[64][0]._ctx
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            for br, pair in sets.items():
                assert _same_bits(m.heldout_score(*pair), ref[br]), (limit, br)
    finally:
        ctx.set_grid_limit(0)
    # a row's score does not depend on its position, its neighbours or the weights: the second half alone, unweighted
    h = n // 2
    half = m.heldout_score(P.SparseDataset.from_dense(train[h:]), P.SparseDataset.from_dense(held[h:]))
    assert np.array_equal(half.llks, ref[n].llks[h:])


# ------------------------------------------------------------------ 5. edges
def test_edge_datasets_and_errors(P, oracle):
    n, d, k = 300, 2000, 10
    x, w, (s, c, mu), train, held, _ = _case(n, d, k)
    m = P.PPCAModel(s, c, mu)
    tsp, hsp = P.SparseDataset.from_dense(train, w), P.SparseDataset.from_dense(held)
    base = m.heldout_score(tsp, hsp)
    # nothing held: zeros, no NaN
    sc = m.heldout_score(tsp, P.SparseDataset(np.zeros(n + 1, dtype=np.int64), [], [], d))
    assert sc.n_entries == 0 and sc.n_rows == 0 and sc.count == 0.0 and sc.llk == 0.0 and np.all(sc.llks == 0.0)
    assert np.all(_cols(sc) == 0.0)
    # train empty, everything held: the closed-form prior predictive
    full = P.SparseDataset.from_dense(x)
    sc = m.heldout_score(P.SparseDataset(np.zeros(n + 1, dtype=np.int64), [], [], d, w), full)
    v = s * s + (c * c).sum(axis=1)
    l = np.where(np.isfinite(x), -0.5 * (H.LN_2PI + np.log(v)[None, :] + (x - mu[None, :]) ** 2 / v[None, :]), 0.0)
    err = _rel_rows(sc.llks, l.sum(axis=1))
    print("prior predictive: rows %.1e (bound %g)" % (err, TOL_OWN))
    assert err <= TOL_OWN and sc.n_entries == full.nnz == int(np.isfinite(x).sum())
    # held = train (not disjoint): scored as a new reading of the column
    sc = m.heldout_score(tsp, P.SparseDataset.from_dense(train))
    errs = _errors(sc, H.score(train, train, s, c, mu, w=w, post=oracle.infer(train, s, c, mu)))
    _show("held = train:", errs, TOL)
    assert max(errs.values()) <= TOL, errs
    # weights: train's count, twice the weights double the sums exactly; held's are ignored
    twice = m.heldout_score(tsp.with_weights(2.0 * w), hsp)
    assert np.array_equal(_cols(twice), 2.0 * _cols(base)) and np.array_equal(twice.llks, base.llks)
    assert _same_bits(m.heldout_score(tsp, hsp.with_weights(np.arange(n) + 0.25)), base)
    # shapes and tilings that differ
    short_rows, short_cols = P.SparseDataset.from_dense(held[:-1]), P.SparseDataset.from_dense(held[:, :-1])
    other_tiling = P.SparseDataset.from_dense(held, block_rows=64)
    for bad in (short_rows, short_cols, other_tiling):
        with pytest.raises(ValueError):
            m.heldout_score(tsp, bad)
    with pytest.raises(ValueError, match="block_rows"):
        m.heldout_score(tsp, other_tiling)
    with pytest.raises(TypeError):
        m.heldout_score(tsp, P.Dataset(held))
    with pytest.raises(TypeError):
        m.heldout_score(P.Dataset(train), hsp)
    with pytest.raises(TypeError):
        m.loo_llk(tsp)
    from ppca_rs_amd import _lib

    tot = np.zeros(6)
    for bad in (short_rows, short_cols, other_tiling):
        rc = _lib.lib().ppca_heldout_score_sparse(tsp._ctx.handle, tsp._sh, bad._sh, m._device(tsp._ctx).h, tot.ctypes.data_as(C.c_void_p), None, None)
        assert rc == INVALID
    x9, w9, _ = SC.case(64, 9, 3)
    t9, h9 = P.SparseDataset.from_dense(x9, w9).holdout(0.3, 1)
    with pytest.raises(P.PPCAError) as err:
        P.PPCAModel(1.0, np.random.default_rng(0).standard_normal((9, 17)), np.zeros(9)).heldout_score(t9, h9)
    assert err.value.code == UNSUPPORTED
    with pytest.raises(TypeError):
        P.heldout_score(P.FAModel(np.ones(9), np.ones((9, 2)), np.zeros(9)), t9, h9)


# ------------------------------------------------------------------ 6. the host split is the device split
@pytest.mark.parametrize("f", [0.1, 0.5])
@pytest.mark.parametrize("n,d,seed", [(300, 65, 13), (130, 300, 15)])
def test_split_parity_with_the_device_split(P, n, d, seed, f):
    x = H.split_data(n, d, seed)
    train, held = P.SparseDataset.from_dense(x).holdout(f, seed)
    dt, dh = P.Dataset(x).holdout(f, seed)
    for got, want in ((train, P.SparseDataset.from_dense(dt.numpy())), (held, P.SparseDataset.from_dense(dh.numpy()))):
        a, b = got.csr(), want.csr()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    assert train.holdout_counts == dt.holdout_counts


# ------------------------------------------------------------------ 7. row shards
def test_shards_add_up(P):
    n, d, k = 300, 2000, 10
    x, w, (s, c, mu), _, _, _ = _case(n, d, k)
    m = P.PPCAModel(s, c, mu)
    whole = m.heldout_score(*P.SparseDataset.from_dense(x, w).holdout(0.3, 17))
    h = n // 2
    a = m.heldout_score(*P.SparseDataset.from_dense(x[:h], w[:h]).holdout(0.3, 17))
    b = m.heldout_score(*P.SparseDataset.from_dense(x[h:], w[h:]).holdout(0.3, 17, row_offset=h))
    both = a + b
    assert np.array_equal(both.llks, whole.llks) and (both.n_entries, both.n_rows) == (whole.n_entries, whole.n_rows)
    _cols_close(both, whole)


# ------------------------------------------------------------------ 8. end to end
def test_select_state_size_on_sparse_data(P, oracle):
    """The pinned case of tests/test_gpu_heldout.py::test_select_state_size_finds_the_true_one (true k = 3; the CPU reference alone
    peaks there, -1.0224 against -1.0315 at k = 4).  The sparse trainer sees the same split and the same random starts as the dense
    one, so the six held-out means agree to the parity bound."""
    x, _, _ = oracle.synth(600, 12, 3, 0.3, 13, sigma_true=0.5)
    sp = P.SparseDataset.from_dense(x)
    out = P.PPCATrainer(sp).select_state_size(range(1, 7), fraction=0.15, seed=7, n_iters=30)
    assert [k for k, _, _ in out] == [1, 2, 3, 4, 5, 6]
    got = np.array([sc.mean_llk for _, sc, _ in out])
    dense = np.array([sc.mean_llk for _, sc, _ in P.PPCATrainer(P.Dataset(x)).select_state_size(range(1, 7), fraction=0.15, seed=7, n_iters=30)])
    err = float((np.abs(got - dense) / (1.0 + np.abs(dense))).max())
    print("held-out mean llk sparse", got.tolist(), "dense", dense.tolist(), "worst %.1e (bound %g)" % (err, TOL))
    assert int(np.argmax(got)) == 2
    assert err <= TOL
    pooled = P.PPCATrainer(sp).select_state_size([2, 3, 4], seed=7, folds=3)
    assert [k for k, _, _ in pooled] == [2, 3, 4] and all(sc.n_entries == sp.nnz for _, sc, _ in pooled)
    assert all(len(models) == 3 for _, _, models in pooled)
    scores, pool, models = P.cross_validate(sp, lambda tr: P.PPCATrainer(tr).train(state_size=3, n_iters=5, quiet=True, seed=7), folds=3, seed=7)
    assert len(scores) == len(models) == 3 and pool.n_entries == sp.nnz and np.isfinite(pool.mean_llk)
    with pytest.raises(ValueError):
        P.PPCATrainer(sp).select_state_size([2], fraction=0.15, seed=7, init="pca")
    with pytest.raises(ValueError):
        P.cross_validate(sp, lambda tr: None, folds=3, seed=7, precisions=np.ones(x.shape))
