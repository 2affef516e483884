"""Held-out scoring of TPPCAModel and HPPCAModel, and K-fold splits, on the GPU: the scores against the numpy
restatement (tests/heldout_families_restatement.py), their reductions to the Gaussian score, the chain rule through the library's own
llks, independence of the launch geometry, the errors, Dataset.kfold against the restated rule bit for bit, and three end-to-end
comparisons of families on identical held entries.

Bounds (those of tests/test_gpu_heldout.py).  TOL = 1e-5, the project's GPU parity tolerance, against the restatement: per row
relative to 1 + |value|, sums relative to the sum of their terms' magnitudes.  TOL_OWN = 1e-10 between two of the library's own routes.
Bit equality where the contract says that a value depends on its row alone.  Every parity check prints its worst error before it
asserts."""
import ctypes as C

import numpy as np
import pytest

import heldout_families_restatement as F
import heldout_restatement as H
import hppca_restatement as HP
import tppca_restatement as TP

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_OWN = 1e-10
# N x d x k: one entry; an odd d below a wave; the fused posterior pass (d = 256, k = 10); k = 16 with a last block of 8 columns;
# the largest (d, k) the two families cover
SCORE_SHAPES = [(1, 1, 1), (200, 31, 6), (300, 256, 10), (200, 200, 16), (100, 1024, 16)]
QS = ("count", "llk", "se", "z2")


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _same_bits(got, want):
    """values and NaN positions"""
    fin = np.isfinite(want)
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[fin].view(np.int64), want[fin].view(np.int64))


def _errors(sc, res):
    """HeldOutScore against a restatement result: per row, column sums and totals"""
    cols = sc.columns
    got = np.stack([cols[q] for q in QS])
    scale = np.where(res["col_abs"] > 0, res["col_abs"], 1.0)
    tot = np.array([sc.count, sc.llk, float(sum(cols["se"].tolist())), float(sum(cols["z2"].tolist()))])  # (index order, as the library's)
    tscale = np.where(res["total_abs"] > 0, res["total_abs"], 1.0)
    rows = float((np.abs(sc.llks - res["per_row"]) / (1.0 + np.abs(res["per_row"]))).max()) if len(res["per_row"]) else 0.0
    return dict(rows=rows, cols=float((np.abs(got - res["col_sums"]) / scale).max()),
                totals=float((np.abs(tot - res["totals"][:4]) / tscale).max()))


def _check(label, sc, res, bound=TOL):
    errs = _errors(sc, res)
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % bound)
    assert sc.n_entries == int(res["totals"][4]) and sc.n_rows == int(res["totals"][5]), label
    assert np.all(np.isfinite(sc.llks)) and max(errs.values()) <= bound, (label, errs)


def _own_close(a, b, label):
    """two of the library's routes: rows and column sums to TOL_OWN"""
    rows = float((np.abs(a.llks - b.llks) / (1.0 + np.abs(b.llks))).max()) if len(b.llks) else 0.0
    cols = max(float((np.abs(a.columns[q] - b.columns[q]) / np.maximum(np.abs(b.columns[q]), 1e-300)).max()) for q in QS)
    print(label, "rows %.1e cols %.1e (bound %g)" % (rows, cols, TOL_OWN))
    assert rows <= TOL_OWN and cols <= TOL_OWN and (a.n_entries, a.n_rows) == (b.n_entries, b.n_rows), label


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------ 1. the scores against the restatement
_T_CASES, _H_CASES = {}, {}


def _t_case(n, d, k, fraction=0.15, mask=True):
    """x (30 % masked unless mask=False), weights, a model near the truth and the split; rows 3, 4, 5 have 0, 1 and 2 train entries (their
    other entries held), row 6 has no held entry (n >= 20).  Computed once per key; read-only."""
    key = (n, d, k, fraction, mask)
    if key not in _T_CASES:
        x, w, (s, c, mu) = TP.masked_case(n, d, k, 40 + d + k)
        if not mask:
            x = np.random.default_rng(d).standard_normal((n, d))
        if n == 1:
            x = np.full((1, d), 0.3)  # (the one entry is there, and held)
        train, held, _ = H.holdout(x, 1.0 if n == 1 else fraction, 60 + d)
        if n >= 20 and d >= 8 and fraction < 1.0:
            for r, keep in ((3, 0), (4, 1), (5, 2)):
                o = np.flatnonzero(np.isfinite(x[r]))
                train[r], held[r] = np.nan, np.nan
                train[r, o[:keep]], held[r, o[keep:]] = x[r, o[:keep]], x[r, o[keep:]]
            train[6], held[6] = np.where(np.isfinite(x[6]), x[6], np.nan), np.nan
        _T_CASES[key] = _frozen(x, w, c, mu, train, held) + (s,)
    return _T_CASES[key]


@pytest.mark.parametrize("nu", [0.7, 4.0, 1e4])
@pytest.mark.parametrize("n,d,k", SCORE_SHAPES)
def test_t_score_matches_the_restatement(P, n, d, k, nu):
    x, w, c, mu, train, held, s = _t_case(n, d, k)
    m, tds, hds = P.TPPCAModel(s, c, mu, nu), P.Dataset(train, w), P.Dataset(held)
    sc = m.score_heldout(tds, hds)
    _check("t %dx%dx%d nu=%g:" % (n, d, k, nu), sc, F.t_score(train, held, s, c, mu, nu, w=w))
    assert np.all(sc.llks[~np.isfinite(held).any(axis=1)] == 0.0)
    again = P.heldout_score(m, tds, hds)  # two runs, the second through the family-wide function: the same bits
    assert np.array_equal(again.llks, sc.llks) and all(np.array_equal(again.columns[q], sc.columns[q]) for q in QS)
    if n >= 20 and d >= 8 and nu == 0.7:
        # the z^2 rule on both sides of nu_m = 2: rows 3 and 4 (nu_m = 0.7, 1.7) have no variance and add exactly 0, row 5 (2.7) adds
        # e^2 (nu_m - 2) / (nu_m s) > 0; all three count everywhere else
        lo, hi = m.score_heldout(tds._slice(3, 2), hds._slice(3, 2)), m.score_heldout(tds._slice(5, 1), hds._slice(5, 1))
        assert lo.n_entries == int(np.isfinite(held[3:5]).sum()) > 0 and lo.n_rows == 2 and lo.llk != 0.0 and lo.mse > 0.0
        assert np.all(lo.columns["z2"] == 0.0) and lo.mean_z2 == 0.0
        assert hi.n_entries > 0 and hi.mean_z2 > 0.0


@pytest.mark.parametrize("nu", [0.7, 1e4])
def test_t_score_when_the_list_flushes_mid_row(P, nu):
    """half of d = 200 held: about 70 entries in a row, so the 64-entry list flushes once mid-row and again with the remainder"""
    n, d, k = 200, 200, 16
    x, w, c, mu, train, held, s = _t_case(n, d, k, fraction=0.5)
    cnt = np.isfinite(held).sum(axis=1)
    assert ((cnt > 64) & (cnt % 64 != 0)).any() and (cnt < 64).any()
    sc = P.TPPCAModel(s, c, mu, nu).score_heldout(P.Dataset(train, w), P.Dataset(held))
    _check("t half held nu=%g:" % nu, sc, F.t_score(train, held, s, c, mu, nu, w=w))


def test_t_score_of_the_prior_predictive(P):
    """fraction 1.0 of a fully observed 60 x 256: the train part is empty, every row gets the t prior predictive (m = 0, delta = 0,
    z = 0, Sigma = I) and lists 4 x 64 entries: four full flushes, no remainder"""
    n, d, k, nu = 60, 256, 10, 4.0
    x, w, c, mu, train, held, s = _t_case(n, d, k, fraction=1.0, mask=False)
    assert not np.isfinite(train).any() and np.isfinite(held).all()
    sc = P.TPPCAModel(s, c, mu, nu).score_heldout(P.Dataset(train, w), P.Dataset(held))
    _check("t prior predictive:", sc, F.t_score(train, held, s, c, mu, nu, w=w))
    v = s * s + (c * c).sum(axis=1)
    l = F.pred_table(0, nu)[0] - 0.5 * np.log(v) - 0.5 * (nu + 1.0) * np.log1p((held - mu) ** 2 / (nu * v))
    assert float((np.abs(sc.llks - l.sum(axis=1)) / (1.0 + np.abs(l.sum(axis=1)))).max()) <= TOL_OWN


def _h_case(n, d, k, fraction=0.15, mask=True):
    """hppca_restatement.case (precisions over 2^-10 .. 2^10, 10 % zeros and 5 % NaN), the split of x, and a SECOND precision array for
    the held part drawn the same way; row 3 has no train entry, row 6 no held entry (n >= 20).  mask=False: x fully observed and every
    precision usable."""
    key = (n, d, k, fraction, mask)
    if key not in _H_CASES:
        x, p, w, (s, c, mu) = HP.case(n, d, k, 70 + d + k)
        q = HP.case(n, d, k, 170 + d + k)[1]
        if not mask:
            rng = np.random.default_rng(d)
            x = rng.standard_normal((n, d))
            p, q = np.exp(rng.uniform(-3.0, 3.0, (n, d))), np.exp(rng.uniform(-3.0, 3.0, (n, d)))
        if n == 1:
            x, p, q = np.full((1, d), 0.3), np.full((1, d), 2.0), np.full((1, d), 0.5)  # (the one entry is there, and held)
        train, held, _ = H.holdout(x, 1.0 if n == 1 else fraction, 80 + d)
        if n >= 20 and fraction < 1.0:
            train[3], held[3] = np.nan, np.where(np.isfinite(x[3]), x[3], np.nan)
            train[6], held[6] = np.where(np.isfinite(x[6]), x[6], np.nan), np.nan
        _H_CASES[key] = _frozen(x, p, q, w, c, mu, train, held) + (s,)
    return _H_CASES[key]


@pytest.mark.parametrize("n,d,k", SCORE_SHAPES)
def test_known_precision_score_matches_the_restatement(P, n, d, k):
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k)
    if n >= 20:  # zeros and NaNs on both sides, at finite values too
        for a, part in ((p, train), (q, held)):
            at = np.isfinite(part)
            assert (a[at] == 0.0).any() and np.isnan(a[at]).any()
    m, tds, hds = P.HPPCAModel(s, c, mu), P.Dataset(train, w), P.Dataset(held)
    sc = m.score_heldout(tds, hds, p, q)
    _check("known precision %dx%dx%d:" % (n, d, k), sc, F.h_score(train, p, held, q, s, c, mu, w=w))
    assert np.all(sc.llks[~HP.observed(held, q).any(axis=1)] == 0.0)
    again = m.score_heldout(tds, hds, P.Dataset(p), P.Dataset(q))  # two runs, the precisions as datasets: the same bits
    assert np.array_equal(again.llks, sc.llks) and all(np.array_equal(again.columns[r], sc.columns[r]) for r in QS)
    same = P.heldout_score(m, tds, hds, p)  # one handle for both sides, through the family-wide function
    _check("known precision %dx%dx%d, one handle:" % (n, d, k), same, F.h_score(train, p, held, p, s, c, mu, w=w))


def test_known_precision_score_when_the_list_flushes_mid_row(P):
    n, d, k = 200, 200, 16
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k, fraction=0.5)
    assert HP.observed(held, q).sum(axis=1).max() > 64
    sc = P.HPPCAModel(s, c, mu).score_heldout(P.Dataset(train, w), P.Dataset(held), p, q)
    _check("known precision half held:", sc, F.h_score(train, p, held, q, s, c, mu, w=w))


def test_known_precision_score_of_the_prior_predictive(P):
    n, d, k = 60, 256, 10
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k, fraction=1.0, mask=False)
    assert not np.isfinite(train).any() and HP.observed(held, q).all()
    sc = P.HPPCAModel(s, c, mu).score_heldout(P.Dataset(train, w), P.Dataset(held), p, q)
    _check("known precision prior predictive:", sc, F.h_score(train, p, held, q, s, c, mu, w=w))
    v = s * s / q + (c * c).sum(axis=1)[None, :]
    l = (-0.5 * (H.LN_2PI + np.log(v) + (held - mu) ** 2 / v)).sum(axis=1)
    assert float((np.abs(sc.llks - l) / (1.0 + np.abs(l))).max()) <= TOL_OWN


# ------------------------------------------------------------------ 2. reductions to the Gaussian score
@pytest.mark.parametrize("n,d,k", [(200, 31, 6), (300, 256, 10), (100, 1024, 16)])
def test_unit_precisions_give_the_gaussian_score(P, n, d, k):
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k)
    m, tds, hds = P.HPPCAModel(s, c, mu), P.Dataset(train, w), P.Dataset(held)
    _own_close(m.score_heldout(tds, hds, np.ones((n, d))), m.gaussian().heldout_score(tds, hds), "precisions 1 %dx%dx%d:" % (n, d, k))
    # precisions in {0, 1}: the Gaussian score of the datasets masked where the precision is 0
    rng = np.random.default_rng(n + d)
    tp, hp = (rng.random((n, d)) < 0.7).astype(np.float64), (rng.random((n, d)) < 0.7).astype(np.float64)
    got = m.score_heldout(tds, hds, tp, hp)
    want = m.gaussian().heldout_score(P.Dataset(np.where(tp > 0, train, np.nan), w), P.Dataset(np.where(hp > 0, held, np.nan)))
    _own_close(got, want, "precisions in {0, 1} %dx%dx%d:" % (n, d, k))


# ------------------------------------------------------------------ 3. the chain rule through the library
def _one_held(x, seed):
    """train / held with exactly one held entry in every row that has an observed one"""
    rng = np.random.default_rng(seed)
    train, held = x.copy(), np.full_like(x, np.nan)
    for i in range(x.shape[0]):
        o = np.flatnonzero(np.isfinite(x[i]))
        if len(o):
            j = o[rng.integers(len(o))]
            held[i, j], train[i, j] = x[i, j], np.nan
    return train, held


def _chain_err(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.parametrize("nu", [0.7, 4.0])
def test_t_score_is_the_chain_rule_of_llks(P, nu):
    n, d, k = 200, 31, 6
    x, w, c, mu, _, _, s = _t_case(n, d, k)
    train, held = _one_held(x, 3)
    m = P.TPPCAModel(s, c, mu, nu)
    want = m.llks(P.Dataset(np.where(np.isfinite(x), x, np.nan))) - m.llks(P.Dataset(train))
    err = _chain_err(m.score_heldout(P.Dataset(train), P.Dataset(held)).llks, want)
    print("t chain rule through llks nu=%g: %.1e (bound %g)" % (nu, err, TOL))
    assert err <= TOL


def test_known_precision_score_is_the_chain_rule_of_llks(P):
    n, d, k = 200, 31, 6
    x, p, _, w, c, mu, _, _, s = _h_case(n, d, k)
    xo = np.where(HP.observed(x, p), x, np.nan)  # (an entry without a usable precision is not there for either side)
    train, held = _one_held(xo, 4)
    m = P.HPPCAModel(s, c, mu)
    want = m.llks(P.Dataset(xo), p) - m.llks(P.Dataset(train), p)
    err = _chain_err(m.score_heldout(P.Dataset(train), P.Dataset(held), p).llks, want)
    print("known-precision chain rule through llks: %.1e (bound %g)" % (err, TOL))
    assert err <= TOL


# ------------------------------------------------------------------ 4. independence of the launch geometry
def _geometry(P, monkeypatch, n, base, score, sliced):
    from ppca_rs_amd import _lib

    def sums_close(sc, label):
        for q in QS:
            scale = np.maximum(np.abs(base.columns[q]), 1e-300)
            assert (np.abs(sc.columns[q] - base.columns[q]) / scale).max() <= TOL_OWN, (label, q)
        assert (sc.n_entries, sc.n_rows) == (base.n_entries, base.n_rows)

    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(3)
        sc = score()
    finally:
        ctx.set_grid_limit(0)
    assert np.array_equal(sc.llks, base.llks)
    sums_close(sc, "grid")
    monkeypatch.setenv("PPCA_HELD_CHUNK", "64")
    sc = score()
    monkeypatch.delenv("PPCA_HELD_CHUNK")
    assert np.array_equal(sc.llks, base.llks)
    sums_close(sc, "chunk")
    s0, ln = n // 3 + 5, n // 2
    assert np.array_equal(sliced(s0, ln).llks, base.llks[s0:s0 + ln])


@pytest.mark.parametrize("n,d,k", [(300, 256, 10), (200, 200, 16)])
def test_scores_do_not_depend_on_grid_chunks_or_slices(P, monkeypatch, n, d, k):
    x, w, c, mu, train, held, s = _t_case(n, d, k)
    m, tds, hds = P.TPPCAModel(s, c, mu, 4.0), P.Dataset(train, w), P.Dataset(held)
    _geometry(P, monkeypatch, n, m.score_heldout(tds, hds), lambda: m.score_heldout(tds, hds),
              lambda s0, ln: m.score_heldout(tds._slice(s0, ln), hds._slice(s0, ln)))
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k)
    m, tds, hds, pds, qds = P.HPPCAModel(s, c, mu), P.Dataset(train, w), P.Dataset(held), P.Dataset(p), P.Dataset(q)
    _geometry(P, monkeypatch, n, m.score_heldout(tds, hds, pds, qds), lambda: m.score_heldout(tds, hds, pds, qds),
              lambda s0, ln: m.score_heldout(tds._slice(s0, ln), hds._slice(s0, ln), pds._slice(s0, ln), qds._slice(s0, ln)))


# ------------------------------------------------------------------ 5. errors and edges
def _raw_h(P, m, tds, pds, hds, qds, tot, cols, rows):
    from ppca_rs_amd import _lib

    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _lib.lib().ppca_h_heldout_score(tds._ctx.handle, tds._h, pds._h, hds._h, qds._h, m._device(tds._ctx).h, vp(tot), vp(cols), vp(rows))


@pytest.mark.parametrize("bad", [-1.0, float("inf")])
def test_a_bad_held_precision_is_refused_with_no_output(P, bad):
    n, d, k = 200, 31, 6
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k)
    i, j = np.argwhere(np.isfinite(held))[17]
    q2 = q.copy()
    q2[i, j] = bad
    m, tds, hds = P.HPPCAModel(s, c, mu), P.Dataset(train, w), P.Dataset(held)
    with pytest.raises(P.PPCAError):
        m.score_heldout(tds, hds, p, q2)
    tot, cols, rows = np.full(6, 7.0), np.full((4, d), 7.0), np.full(n, 7.0)
    assert _raw_h(P, m.gaussian(), tds, P.Dataset(p), hds, P.Dataset(q2), tot, cols, rows) == -1  # PPCA_ERR_INVALID
    assert np.all(tot == 7.0) and np.all(cols == 7.0) and np.all(rows == 7.0)
    # the same value where the held x is NaN is not an error: the entry is not observed
    i, j = np.argwhere(~np.isfinite(held))[5]
    q3 = q.copy()
    q3[i, j] = bad
    a, b = m.score_heldout(tds, hds, p, q3), m.score_heldout(tds, hds, p, q)
    assert np.array_equal(a.llks, b.llks)
    # a bad TRAIN precision is the sweep's error, as in every other pass of the class
    p2 = p.copy()
    p2[0, 0] = bad
    with pytest.raises(P.PPCAError):
        m.score_heldout(tds, hds, p2, q)


def test_sizes_beyond_the_families_are_unsupported(P):
    from ppca_rs_amd import _lib

    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(2)
    for n, d, k in ((8, 40, 17), (4, 1025, 3)):
        x = rng.standard_normal((n, d))
        g = P.PPCAModel(0.5, rng.standard_normal((d, k)), np.zeros(d))
        tds, hds, one = P.Dataset(x), P.Dataset(x), P.Dataset(np.ones((n, d)))
        tot = np.full(6, 7.0)
        h = g._device(tds._ctx).h
        assert _lib.lib().ppca_t_heldout_score(tds._ctx.handle, tds._h, hds._h, h, 4.0, vp(tot), None, None) == -3  # PPCA_ERR_UNSUPPORTED
        assert _lib.lib().ppca_h_heldout_score(tds._ctx.handle, tds._h, one._h, hds._h, one._h, h, vp(tot), None, None) == -3
        assert np.all(tot == 7.0)


def test_shape_mismatch_and_empty_datasets(P):
    n, d, k = 200, 31, 6
    x, p, q, w, c, mu, train, held, s = _h_case(n, d, k)
    hm, tm = P.HPPCAModel(s, c, mu), P.TPPCAModel(s, c, mu, 4.0)
    tds, hds = P.Dataset(train, w), P.Dataset(held)
    with pytest.raises(ValueError):
        tm.score_heldout(tds, P.Dataset(held[:-1]))
    with pytest.raises(ValueError):
        hm.score_heldout(tds, P.Dataset(held[:-1]), p)
    with pytest.raises(ValueError):
        hm.score_heldout(tds, hds, p[:-1])
    with pytest.raises(ValueError):
        hm.score_heldout(tds, hds, p, q[:, :-1])
    tot = np.zeros(6)
    short = P.Dataset(np.ascontiguousarray(q[:-1]))
    assert _raw_h(P, hm.gaussian(), tds, P.Dataset(p), hds, short, tot, np.zeros((4, d)), np.zeros(n)) == -1
    empty = np.empty((0, d))
    for sc in (tm.score_heldout(P.Dataset(empty), P.Dataset(empty)), hm.score_heldout(P.Dataset(empty), P.Dataset(empty), empty)):
        assert sc.n_entries == 0 and sc.n_rows == 0 and sc.count == 0.0 and sc.llk == 0.0 and len(sc.llks) == 0
        assert all(np.all(sc.columns[r] == 0.0) for r in QS)
    # nothing held: zeros, no NaN
    sc = tm.score_heldout(tds, P.Dataset(np.full((n, d), np.nan)))
    assert sc.n_entries == 0 and sc.llk == 0.0 and np.all(sc.llks == 0.0)


# ------------------------------------------------------------------ 6. folds
@pytest.mark.parametrize("n_folds", [2, 5])
@pytest.mark.parametrize("n,d,seed", [(5, 63, 11), (300, 65, 13), (257, 256, 14), (70, 1024, 16)])
def test_kfold_matches_the_restated_rule(P, n, d, seed, n_folds):
    x = H.split_data(n, d, seed)
    w = np.random.default_rng(seed).uniform(0.25, 2.0, n)
    ds = P.Dataset(x, w)
    obs = np.isfinite(x)
    times = np.zeros((n, d), dtype=np.int64)
    folds = ds.kfold(n_folds, seed)
    assert len(folds) == n_folds
    for (train, held), (want_t, want_h, counts) in zip(folds, F.kfold(x, n_folds, seed)):
        gh = held.numpy()
        assert _same_bits(train.numpy(), want_t) and _same_bits(gh, want_h)
        assert train.holdout_counts == counts and held.holdout_counts == counts and sum(counts) == int(obs.sum())
        assert np.array_equal(train.weights(), w) and np.array_equal(held.weights(), w)
        times += np.isfinite(gh)
    assert np.array_equal(times, obs.astype(np.int64))  # every observed entry in exactly one fold
    if n >= 3:  # a shard with its row offset reproduces its rows
        s0, ln = n // 3, n - n // 3 - 1
        for (ts, hs), (want_t, want_h, _) in zip(ds._slice(s0, ln).kfold(n_folds, seed, row_offset=s0), F.kfold(x, n_folds, seed)):
            assert _same_bits(ts.numpy(), want_t[s0:s0 + ln]) and _same_bits(hs.numpy(), want_h[s0:s0 + ln])


def test_a_range_from_zero_is_the_fraction_split(P):
    from ppca_rs_amd import _lib

    x = H.split_data(257, 256, 14)
    ds = P.Dataset(x)
    for f in H.SPLIT_FRACTIONS:
        (ta, ha), (tb, hb) = ds.holdout_range(0.0, f, 14), ds.holdout(f, 14)
        assert _same_bits(ta.numpy(), tb.numpy()) and _same_bits(ha.numpy(), hb.numpy()) and ta.holdout_counts == tb.holdout_counts
    want_t, want_h, counts = F.holdout_range(x, 0.25, 0.6, 14)
    t, h = ds.holdout_range(0.25, 0.6, 14)
    assert _same_bits(t.numpy(), want_t) and _same_bits(h.numpy(), want_h) and t.holdout_counts == counts
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.5), (float("nan"), 0.5), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            ds.holdout_range(lo, hi, 1)
        th, hh = C.c_void_p(), C.c_void_p()
        rc = _lib.lib().ppca_dataset_holdout_range(ds._ctx.handle, ds._h, lo, hi, 1, 0, C.byref(th), C.byref(hh), None)
        assert rc == -1 and not th.value and not hh.value  # PPCA_ERR_INVALID, nothing allocated
    with pytest.raises(ValueError):
        ds.kfold(1, 1)
    with pytest.raises(ValueError):
        ds.kfold(3, 1, row_offset=-1)


# ------------------------------------------------------------------ 7. families compared on identical held entries
def test_the_t_fit_predicts_contaminated_data_better(P):
    """tppca_restatement's contaminated case (N = 600, d = 12, k = 3, 5 % gross rows), five folds of seed 7, 30 iterations per fit.  The
    CPU alone (the oracle's Gaussian EM and the restated t ECM from the same start, scored by the restatements) gives a pooled held-out
    mean log-density of -2.8721 for the Gaussian fit and -1.3180 for the t fit (dof = 4), the t fit ahead in each of the five folds; the
    library's fits start elsewhere (PPCAModel.init), and only the ordering is asserted."""
    ds = P.Dataset(TP.contaminated_start()[0])
    _, gauss, _ = P.cross_validate(ds, lambda tr: P.PPCATrainer(tr).train(state_size=3, n_iters=30, quiet=True, seed=1), folds=5, seed=7)
    scores, t, models = P.cross_validate(ds, lambda tr: P.TPPCATrainer(tr).train(state_size=3, dof=4.0, n_iters=30, quiet=True, seed=1),
                                         folds=5, seed=7)
    print("contaminated, pooled held-out mean llk: gaussian %.4f, t %.4f" % (gauss.mean_llk, t.mean_llk))
    assert len(scores) == 5 and len(models) == 5 and all(isinstance(m, P.TPPCAModel) for m in models)
    assert t.n_entries == gauss.n_entries == int(np.isfinite(ds.numpy()).sum())  # every observed entry held exactly once, in both
    assert t.mean_llk > gauss.mean_llk


def test_the_true_precisions_predict_better(P):
    """hppca_restatement.hetero_case() (N = 600, d = 12, k = 3, noise levels 0.3 and 3.0), five folds of seed 7, 30 iterations per fit.
    The CPU alone (the oracle's Gaussian EM and the restated ECM from the same start) gives a pooled held-out mean log-density of
    -2.3099 for the Gaussian fit and -1.7468 for the fit and score with the true precisions; only the ordering is asserted."""
    x, p, _, _ = HP.hetero_case()
    ds = P.Dataset(x)
    _, gauss, _ = P.cross_validate(ds, lambda tr: P.PPCATrainer(tr).train(state_size=3, n_iters=30, quiet=True, seed=1), folds=5, seed=7)
    _, known, models = P.cross_validate(ds, lambda tr, pr: P.HPPCATrainer(tr, pr).train(state_size=3, n_iters=30, seed=1), folds=5, seed=7,
                                        precisions=p)
    print("hetero, pooled held-out mean llk: gaussian %.4f, known precisions %.4f" % (gauss.mean_llk, known.mean_llk))
    assert all(isinstance(m, P.HPPCAModel) for m in models) and known.n_entries == gauss.n_entries
    assert known.mean_llk > gauss.mean_llk


def test_t_selection_with_folds_finds_the_true_state_size(P, oracle):
    """the pinned selection case of tests/test_gpu_heldout.py (true k = 3, N = 600, d = 12, 30 % masked, noise 0.5)"""
    x, _, _ = oracle.synth(600, 12, 3, 0.3, 13, sigma_true=0.5)
    out = P.TPPCATrainer(P.Dataset(x)).select_state_size(range(1, 6), folds=3, seed=7, n_iters=30)
    held = [sc.mean_llk for _, sc, _ in out]
    print("t selection, pooled held-out mean llk per size", held)
    assert [k for k, _, _ in out] == [1, 2, 3, 4, 5] and all(len(ms) == 3 for _, _, ms in out)
    assert all(sc.n_entries == int(np.isfinite(x).sum()) for _, sc, _ in out)
    assert int(np.argmax(held)) == 2
    hp = P.HPPCATrainer(P.Dataset(x), np.ones_like(x)).select_state_size([2, 3], fraction=0.15, seed=7, n_iters=5)
    assert [k for k, _, _ in hp] == [2, 3] and all(np.isfinite(sc.mean_llk) and isinstance(m, P.HPPCAModel) for _, sc, m in hp)
