"""Factor analysis on row-compressed data on the GPU: the device-side rescaling of a SparseDataset against numpy;
FAModel on a SparseDataset against the dense restatement in the original units (tests/fa_restatement.py), against the library's dense
path and against the held-out restatement; what the design promises exactly; behaviour of the loop; errors.

Cases: tests/sparse_fa_cases.py::CASES -- the eight shapes at the default tiling, the state-size sweep k = 0 .. 16 at (150, 300) under
block_rows = 64, segment = 8, and the seam shape (300, 300, 4) under four tilings.  No case and no column is left out of a comparison.

Bounds.  TOL = 1e-5, the project's GPU parity bound, with the measures of tests/test_gpu_factor_noise.py (psi per element; C against
max |C|; mean_j against max(|mean_j|, psi_j); a row's llk against |llk| + d) against the restatement and those of
tests/test_gpu_sparse.py::_check_against_dense_path against the dense path; TOL_OWN = 1e-10 between the two device paths of the held-out
score (tests/test_gpu_sparse_heldout.py); 1e-12 of the sum of the terms' magnitudes for the sums of the scale pass
(tests/test_gpu_factor_noise.py::test_scale_pass_against_numpy).  Every check prints its worst error before asserting.

The reference of llks is fa_restatement.llks on every row whose m x m covariance can be formed and the same density through the k x k
matrix (sparse_fa_cases.llks_low_rank) on the one row that cannot: row 0 of (40, 70000, 3), 69 999 entries, 39 GB as a covariance.
tests/test_sparse_fa_host.py holds the two forms to each other at 1e-10."""
import functools

import numpy as np
import pytest

import fa_restatement as R
import heldout_restatement as H
import sparse_fa_cases as F
from test_gpu_heldout import _counts_match, _errors, _rel_rows, _rel_sums

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_OWN = 1e-10
INVALID, UNSUPPORTED, EMPTY = -1, -3, -4
IDS = [F.case_id(c) for c in F.CASES]
DENSE = [c for c in F.CASES if c[1] <= 2000]
DENSE_IDS = [F.case_id(c) for c in DENSE]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _arrays(m):
    return m.noise, m.transform, m.mean


def _model_errors(got, want, zero=None):
    """tests/test_gpu_factor_noise.py::_model_errors, with a transform that may have no column (k = 0).  zero: the columns whose new
    variance is exactly 0 (sparse_fa_cases.zero_variance_columns: k = 0 only), where psi has no relative error and the callers hold
    the outcome to zero_variance_outcome instead; C and the mean are compared on every column."""
    (p1, c1, m1), (p0, c0, m0) = got, want
    keep = np.ones(p0.shape, dtype=bool) if zero is None else ~zero
    cerr = float(np.abs(c1 - c0).max() / (np.abs(c0).max() or 1.0)) if c0.size else 0.0
    return dict(psi=float(np.abs(p1 / p0 - 1)[keep].max()) if keep.any() else 0.0, C=cerr,
                mean=float((np.abs(m1 - m0) / np.maximum(np.abs(m0), np.where(keep, p0, 0.0))).max()))


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _show(label, errs, bound):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % bound)


def _sparse(P, n, d, k, tiling, weighted=True):
    x, w, _, _ = F.fa_case(n, d, k)
    return P.SparseDataset.from_dense(x, w if weighted else None, **tiling)


# ------------------------------------------------------------------ 1. the scale pass
@functools.lru_cache(maxsize=None)
def _pass_case(n, d, k):
    """The per-column vectors of a pass (a of both signs) and the numpy sums over the dense form, with the sums of the terms'
    magnitudes.  Shared and read-only."""
    x, w, _, _ = F.fa_case(n, d, k)
    rng = np.random.default_rng(9000 + 31 * n + 7 * d + k)
    a = rng.uniform(0.2, 5.0, d) * rng.choice([-1.0, 1.0], d)
    b, l = rng.standard_normal(d), rng.standard_normal(d)
    obs = np.isfinite(x)
    out = {}
    for name, wt in (("weighted", w), ("plain", np.ones(n))):
        e = np.where(obs, x * a - b, 0.0)
        wm = wt[:, None] * obs
        sums = np.stack([wm.sum(0), (wm * e).sum(0), (wm * e * e).sum(0)])
        out[name] = (sums, np.stack([sums[0], (wm * np.abs(e)).sum(0), sums[2]]))
    lo = np.where(obs, l, 0.0)
    res = dict(a=a, b=b, l=l, obs=obs, rows=lo.sum(1), rows_scale=np.abs(lo).sum(1), **out)
    _freeze(a, b, l, obs, res["rows"], res["rows_scale"], *out["weighted"], *out["plain"])
    return res


@pytest.mark.parametrize("n,d,k,tiling", F.CASES, ids=IDS)
def test_scale_pass_against_numpy(P, n, d, k, tiling):
    x, w, _, _ = F.fa_case(n, d, k)
    e = _pass_case(n, d, k)
    a, b, l = e["a"], e["b"], e["l"]
    sp = _sparse(P, n, d, k, tiling)
    indptr, indices, values = sp.csr()
    view, sums, rows = sp._scale_columns(a, b, l, col_sums=True, row_sums=True)
    assert isinstance(view, P.SparseDataset) and view._handle is not None and view._vals is None  # made on the device, nothing fetched
    vp, vi, vv = view.csr()
    assert np.array_equal(vv, values * a[indices])  # the same single rounding, bit for bit
    assert np.array_equal(vp, indptr) and np.array_equal(vi, indices) and np.array_equal(view.weights(), w)
    assert (view._block_rows, view._segment, view.nnz, len(view)) == (sp._block_rows, sp._segment, sp.nnz, n)
    dense = view.to_dense().numpy()
    assert np.array_equal(dense[e["obs"]], (x * a)[e["obs"]]) and np.isnan(dense[~e["obs"]]).all()
    want, scale = e["weighted"]
    errs = dict(cols=float((np.abs(sums - want) / np.where(scale > 0, scale, 1.0)).max()),
                rows=float((np.abs(rows - e["rows"]) / np.where(e["rows_scale"] > 0, e["rows_scale"], 1.0)).max()))
    _show("scale pass %s:" % F.case_id((n, d, k, tiling)), errs, 1e-12)
    assert max(errs.values()) <= 1e-12, errs
    assert np.all(sums[:, scale[0] == 0] == 0.0) and np.all(rows[~e["obs"].any(axis=1)] == 0.0)
    # the sums-only forms: the same bits, no view; b and l nullable; two runs give the same bits
    none, sums2, rows2 = sp._scale_columns(a, b, l, out=False, col_sums=True, row_sums=True)
    assert none is None and np.array_equal(sums2, sums) and np.array_equal(rows2, rows)
    assert np.array_equal(sp._scale_columns(a, b, out=False, col_sums=True)[1], sums)
    assert np.array_equal(sp._scale_columns(a, l=l, out=False, row_sums=True)[2], rows)
    assert np.array_equal(sp._scale_columns(a, out=False, col_sums=True)[1][0], sums[0])
    again, sums3, rows3 = sp._scale_columns(a, b, l, col_sums=True, row_sums=True)
    assert np.array_equal(again.csr()[2], vv) and np.array_equal(sums3, sums) and np.array_equal(rows3, rows)
    # a view of a view, and a view under other weights, share the index: values times a again; the un-weighted totals are counts
    twice = view._scale_columns(a)[0]
    assert np.array_equal(twice.csr()[2], vv * a[indices])
    plain, psums, _ = view.with_weights(np.ones(n))._scale_columns(1.0 / a, col_sums=True)
    assert np.array_equal(psums[0], e["obs"].sum(axis=0)) and np.array_equal(plain.weights(), np.ones(n))
    assert np.array_equal(plain.csr()[2], vv * (1.0 / a)[indices])


def test_scale_pass_bits_do_not_depend_on_tiling_weights_or_grid(P):
    n, d, k = F.SEAM
    x, w, _, _ = F.fa_case(n, d, k)
    e = _pass_case(n, d, k)
    a, b, l = e["a"], e["b"], e["l"]
    base = _sparse(P, n, d, k, {})
    view, sums, rows = base._scale_columns(a, b, l, col_sums=True, row_sums=True)
    values = view.csr()[2]
    ctx = base._ctx
    try:
        for tiling in ({},) + F.SEAM_TILINGS:
            for weighted in (True, False):
                sp = _sparse(P, n, d, k, tiling, weighted)
                ref = None
                for limit in (0, 1, 3):
                    ctx.set_grid_limit(limit)
                    v, s, r = sp._scale_columns(a, b, l, col_sums=True, row_sums=True)
                    assert np.array_equal(v.csr()[2], values) and np.array_equal(r, rows), (tiling, weighted, limit)
                    ref = s if ref is None else ref
                    assert np.array_equal(s, ref), (tiling, weighted, limit, "column sums under a grid limit")
                    assert np.array_equal(sp._scale_columns(a, b, out=False, col_sums=True)[1], ref)
                want, scale = e["weighted" if weighted else "plain"]
                assert (np.abs(ref - want) / np.where(scale > 0, scale, 1.0)).max() <= 1e-12
    finally:
        ctx.set_grid_limit(0)
    # a row's sum does not depend on its position or its neighbours: the second half alone
    half = P.SparseDataset.from_dense(x[150:])
    hv, _, hr = half._scale_columns(a, l=l, row_sums=True)
    assert np.array_equal(hr, rows[150:]) and np.array_equal(hv.csr()[2], values[base.csr()[0][150]:])


def test_scale_pass_on_an_empty_dataset(P):
    sp = P.SparseDataset([0], [], [], 5)
    view, sums, rows = sp._scale_columns(np.ones(5), np.ones(5), np.ones(5), col_sums=True, row_sums=True)
    assert len(view) == 0 and view.nnz == 0 and view.csr()[2].shape == (0,) and np.array_equal(sums, np.zeros((3, 5))) and rows.shape == (0,)
    tot, mean, var = sp.column_stats()
    assert not tot.any() and not mean.any() and not var.any()
    rowless = P.SparseDataset(np.zeros(4, dtype=np.int64), [], [], 5)  # rows, but no entry
    view, sums, rows = rowless._scale_columns(np.ones(5), l=np.ones(5), col_sums=True, row_sums=True)
    assert view.nnz == 0 and not sums.any() and np.array_equal(rows, np.zeros(3))


@pytest.mark.parametrize("n,d,k,tiling", [c for c in F.CASES if not c[3]] + [(*F.SEAM, F.SEAM_TILINGS[0])])
def test_column_stats_match_numpy(P, n, d, k, tiling):
    x, w, _, _ = F.fa_case(n, d, k)
    tot, mean, var = _sparse(P, n, d, k, tiling).column_stats()
    obs = np.isfinite(x)
    wm = w[:, None] * obs
    t0 = wm.sum(0)
    live = t0 > 0
    safe = np.where(live, t0, 1.0)
    m0 = np.where(live, (wm * np.where(obs, x, 0.0)).sum(0) / safe, 0.0)
    v0 = np.where(live, (wm * np.where(obs, x - m0, 0.0) ** 2).sum(0) / safe, 0.0)
    # A column with ONE entry of positive weight has variance exactly 0: numpy and the device each return their own rounding of
    # (x - mean)^2 with mean = (w x) / w within an ulp of x, at most (2 u |x|)^2 -- held to (1e-15 |x|)^2; the others relatively.
    single = (obs & (w[:, None] > 0)).sum(0) == 1
    many = live & ~single
    errs = dict(tot=float((np.abs(tot - t0) / safe).max()), mean=float((np.abs(mean - m0) / (np.abs(m0) + np.sqrt(v0) + ~live)).max()),
                var=float((np.abs(var - v0) / np.where(v0 > 0, v0, 1.0))[many].max()) if many.any() else 0.0)
    _show("column stats %dx%dx%d (%d single-entry columns):" % (n, d, k, int(single.sum())), errs, 1e-10)
    assert errs["tot"] <= 1e-12 and errs["mean"] <= 1e-12 and errs["var"] <= 1e-10  # the bounds of the dense test of the same name
    assert np.all(var[single] <= (1e-15 * np.abs(m0[single])) ** 2) and np.all(var >= 0.0)
    assert np.all(tot[~live] == 0) and np.all(mean[~live] == 0) and np.all(var[~live] == 0)


# ------------------------------------------------------------------ 2. against the restatement
@functools.lru_cache(maxsize=None)
def _want(n, d, k):
    """The restatement's llks, one step and one step under a floor, in the original units.  Shared and read-only."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    llks = F.restatement_llks(x, noise, c, mu)
    step = R.iterate(x, w, noise, c, mu)
    floor = np.zeros(d)
    floor[::3] = 2.0 * step[0][::3]  # above the new noise on every third column, 0 elsewhere
    bound = R.iterate(x, w, noise, c, mu, floor)
    _freeze(llks, floor, *step, *bound)
    return dict(llks=llks, step=step, floor=floor, bound=bound)


@pytest.mark.parametrize("n,d,k,tiling", F.CASES, ids=IDS)
def test_against_the_restatement(P, n, d, k, tiling):
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    e = _want(n, d, k)
    sp = _sparse(P, n, d, k, tiling)
    model = P.FAModel(noise, c, mu)
    got = model.llks(sp)
    tot, want_tot, scale = model.llk(sp), float(w @ e["llks"]), float(w @ (np.abs(e["llks"]) + d))
    errs = dict(llks=float((np.abs(got - e["llks"]) / (np.abs(e["llks"]) + d)).max()), llk=abs(tot - want_tot) / scale)
    zero = F.zero_variance_columns(x, w, k)
    new, llk = model.iterate_with_llk(sp)
    errs.update(_model_errors(_arrays(new), e["step"], zero))
    errs.update(step_llk=abs(llk - want_tot) / scale, step_llk_vs_llk=abs(llk - tot) / scale)
    bound = model.iterate(sp, min_noise=e["floor"])
    errs.update({"floor_" + key: v for key, v in _model_errors(_arrays(bound), e["bound"], zero).items()})
    _show("restatement %s:" % F.case_id((n, d, k, tiling)), errs, TOL)
    assert max(errs.values()) <= TOL, errs
    assert F.zero_variance_outcome(new.noise, noise, x, w, mu, zero) and F.zero_variance_outcome(bound.noise, noise, x, w, mu, zero, e["floor"])
    assert np.all(got[~np.isfinite(x).any(axis=1)] == 0.0) and new.state_size == k
    assert np.all(bound.noise >= e["floor"]) and np.array_equal(bound.noise[1::3], new.noise[1::3])
    plain = model.iterate(sp)  # without the llk: the same bits
    assert all(np.array_equal(u, v) for u, v in zip(_arrays(plain), _arrays(new)))
    inf = model.infer(sp)
    assert inf.states().shape == (n, k) and len(inf.covariances()) == n


# ------------------------------------------------------------------ 3. against the dense path
def _dense_model_errors(a, b, zero=None):
    cmax = np.abs(b.transform).max() if b.transform.size else 1.0
    keep = np.ones(b.noise.shape, dtype=bool) if zero is None else ~zero
    return dict(psi=float(np.abs(a.noise / b.noise - 1)[keep].max()) if keep.any() else 0.0,
                C=float(np.abs(a.transform - b.transform).max() / (cmax or 1.0)) if b.transform.size else 0.0,
                mean=float((np.abs(a.mean - b.mean) / np.maximum(np.abs(b.mean), b.noise)).max()))


@pytest.mark.parametrize("n,d,k,tiling", DENSE, ids=DENSE_IDS)
def test_against_the_dense_path(P, n, d, k, tiling):
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    sp = _sparse(P, n, d, k, tiling)
    ds = sp.to_dense()
    assert np.array_equal(np.isfinite(ds.numpy()), np.isfinite(x)) and np.array_equal(ds.weights(), w)
    model = P.FAModel(noise, c, mu)
    dl = model.llks(ds)
    errs = dict(llks=_rel(model.llks(sp), dl), llk=abs(model.llk(sp) - model.llk(ds)) / max(float(np.abs(w * dl).sum()), 1.0))
    if k > 0:
        a, b = model.infer(sp), model.infer(ds)
        errs.update(z=_rel(a.states(), b.states()), Sigma=_rel(np.array(a.covariances()), np.array(b.covariances())))
    (new_s, llk_s), (new_d, llk_d) = model.iterate_with_llk(sp), model.iterate_with_llk(ds)
    zero = F.zero_variance_columns(x, w, k)
    errs.update({"it_" + key: v for key, v in _dense_model_errors(new_s, new_d, zero).items()})
    errs["it_llk"] = abs(llk_s - llk_d) / max(float(np.abs(w * dl).sum()), 1.0)
    _show("dense path %s:" % F.case_id((n, d, k, tiling)), errs, TOL)
    assert max(errs.values()) <= TOL, errs
    assert F.zero_variance_outcome(new_s.noise, noise, x, w, mu, zero)  # (the dense step's own rounding there is not this file's subject)
    assert new_s.state_size == k


@functools.lru_cache(maxsize=None)
def _held_case(n, d, k):
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    train, held, counts = H.holdout(x, 0.3, 50 + d)
    res = H.fa_score(train, held, noise, c, mu, w=w)
    _freeze(train, held, *[v for v in res.values()])
    return train, held, counts, res


def _cols(sc):
    return np.stack([sc.columns[q] for q in ("count", "llk", "se", "z2")])


@pytest.mark.parametrize("n,d,k,tiling", F.CASES, ids=IDS)
def test_heldout_score(P, n, d, k, tiling):
    """FAModel.heldout_score on the two sparse parts against heldout_restatement.fa_score at TOL and (d <= 2000) against the same call
    on the two dense parts at TOL_OWN."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    train, held, counts, res = _held_case(n, d, k)
    model = P.FAModel(noise, c, mu)
    tsp, hsp = P.SparseDataset.from_dense(train, w, **tiling), P.SparseDataset.from_dense(held, **tiling)
    assert (tsp.nnz, hsp.nnz) == counts
    sc = model.heldout_score(tsp, hsp)
    errs = _errors(sc, res)
    _show("held-out %s vs the restatement:" % F.case_id((n, d, k, tiling)), errs, TOL)
    assert _counts_match(sc, res) and sc.n_entries == hsp.nnz and np.all(np.isfinite(sc.llks))
    assert max(errs.values()) <= TOL, errs
    assert np.all(sc.llks[~np.isfinite(held).any(axis=1)] == 0.0)
    again = model.heldout_score(tsp, hsp)
    assert np.array_equal(again.llks, sc.llks) and np.array_equal(_cols(again), _cols(sc))
    if d <= 2000:
        de = model.heldout_score(P.Dataset(train, w), P.Dataset(held))
        scale = np.where(res["col_abs"] > 0, res["col_abs"], 1.0)
        own = dict(rows=_rel_rows(sc.llks, de.llks), cols=_rel_sums(_cols(sc), _cols(de), scale))
        _show("   vs the dense path:", own, TOL_OWN)
        assert max(own.values()) <= TOL_OWN, own
        assert (sc.n_entries, sc.n_rows) == (de.n_entries, de.n_rows)


@pytest.mark.parametrize("n,d,k,tiling", F.CASES, ids=IDS)
def test_predict(P, n, d, k, tiling):
    """(mean, variance) of a new reading at the held positions and at the train part's own, against fa_restatement.posterior applied
    per row: mean_j + c_j . z, c_j^T Sigma c_j + psi_j^2."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    train, held, _, _ = _held_case(n, d, k)
    model = P.FAModel(noise, c, mu)
    tsp = P.SparseDataset.from_dense(train, w, **tiling)
    post = [R.posterior(row, noise, c, mu) for row in train]
    errs = {}
    for name, q in (("held", np.isfinite(held)), ("own", np.isfinite(train))):
        rows, cols = np.nonzero(q)
        indptr = np.concatenate([[0], np.cumsum(q.sum(axis=1))])
        mean, var = model.predict(tsp, (indptr, cols))
        z = np.array([post[i][0] for i in rows]).reshape(rows.size, k)
        S = np.array([post[i][1] for i in rows]).reshape(rows.size, k, k)
        want_mean = mu[cols] + np.einsum("ea,ea->e", c[cols], z)
        want_var = np.einsum("ea,eab,eb->e", c[cols], S, c[cols]) + noise[cols] ** 2
        errs[name + "_mean"], errs[name + "_var"] = _rel(mean / noise[cols], want_mean / noise[cols]), _rel(var / noise[cols] ** 2, want_var / noise[cols] ** 2)
        assert mean.shape == var.shape == (rows.size,)
    _show("predict %s:" % F.case_id((n, d, k, tiling)), errs, TOL)
    assert max(errs.values()) <= TOL, errs
    m2, v2 = model.predict(tsp, P.SparseDataset.from_dense(held))  # a SparseDataset as the query: its pattern
    rows, cols = np.nonzero(np.isfinite(held))
    indptr = np.concatenate([[0], np.cumsum(np.isfinite(held).sum(axis=1))])
    m1, v1 = model.predict(tsp, (indptr, cols))
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2)


# ------------------------------------------------------------------ 4. exactness the design promises
EXACT = [(64, 9, 3, {}), (150, 300, 11, {}), (*F.SEAM, F.SEAM_TILINGS[0]), (100, 20, 0, {})]


@pytest.mark.parametrize("n,d,k,tiling", EXACT, ids=[F.case_id(c) for c in EXACT])
def test_power_of_two_units_are_exact(P, n, d, k, tiling):
    """Columns 7 (an entry in every non-empty row) and 2 multiplied by 2^10 and 2^-10, and the model's noise, rows of C, means and
    floor with them: the whitened view holds the same bits, one step returns psi, C, mean scaled by exactly those factors, and the
    returned llk moves by - sum_j tot_j p_j ln 2."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    f = np.ones(d)
    f[7], f[2] = 2.0 ** 10, 2.0 ** -10
    sp, sps = P.SparseDataset.from_dense(x, w, **tiling), P.SparseDataset.from_dense(x * f, w, **tiling)
    m, ms = P.FAModel(noise, c, mu), P.FAModel(noise * f, c * f[:, None], mu * f)
    va, vb = m._whiten(sp)[0], ms._whiten(sps)[0]
    assert np.array_equal(va.csr()[2], vb.csr()[2])
    floor = 1e-3 * np.sqrt(sp.column_stats()[2])
    (new, llk), (news, llks) = m.iterate_with_llk(sp, floor), ms.iterate_with_llk(sps, floor * f)
    assert np.array_equal(news.noise, new.noise * f) and np.array_equal(news.transform, new.transform * f[:, None])
    assert np.array_equal(news.mean, new.mean * f)
    tot = sp.column_stats()[0]
    p = np.log2(f)
    terms = np.concatenate([[m.whitened().llk(va)], tot * np.log(noise), tot * p * np.log(2.0)])
    err = abs(llks - (llk - float(np.sum(tot * p) * np.log(2.0)))) / float(np.abs(terms).sum())
    print("llk shift %s: %.2e (bound 1e-12)" % (F.case_id((n, d, k, tiling)), err))
    assert err <= 1e-12
    # two runs of a step give the same bits
    again, llk2 = m.iterate_with_llk(sp, floor)
    assert llk2 == llk and all(np.array_equal(u, v) for u, v in zip(_arrays(again), _arrays(new)))


@pytest.mark.parametrize("n,d,k,tiling", EXACT, ids=[F.case_id(c) for c in EXACT])
def test_from_ppca_llks_equal_the_isotropic_models(P, n, d, k, tiling):
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    sp = P.SparseDataset.from_dense(x, w, **tiling)
    m = P.PPCAModel(0.7, c, mu)
    want, got = m.llks(sp), P.FAModel.from_ppca(m).llks(sp)
    err = float((np.abs(got - want) / (np.abs(want) + d)).max())
    print("from_ppca llks %s: %.2e (bound %g)" % (F.case_id((n, d, k, tiling)), err, TOL))
    assert err <= TOL


# ------------------------------------------------------------------ 5. behaviour
# (start, n, d, k) -> the smallest of the 24 steps of the CPU restatement (fa_restatement.iterate / llks) from that start; there the
# floor is active on no column and |llk| <= 5.9e5, so a step's rounding is some 1e-10 and cannot turn one of these
MONOTONE = {("init", 300, 300, 4): 0.9415, ("init", 150, 300, 11): 1.141, ("normal", 300, 300, 4): 0.3535, ("normal", 150, 300, 11): 2.736}


@pytest.mark.parametrize("start,n,d,k", list(MONOTONE), ids=["%s-%dx%dx%d" % c for c in MONOTONE])
def test_llk_never_decreases(P, start, n, d, k):
    """25 steps from a random start of seed 7 (noise 1, mean 0) under FATrainer's floor: "init" is FAModel.init(k, sp, seed=7), whose
    transform is the reference's column-major fill of the draw; "normal" is default_rng(7).standard_normal((d, k)) with the rows of
    empty columns zeroed.  The two are different starts, hence different trajectories; MONOTONE holds the restatement's smallest step
    of each, and the device's is printed beside it."""
    x, w, _, _ = F.fa_case(n, d, k)
    sp = _sparse(P, n, d, k, {})
    floor = 1e-3 * np.sqrt(sp.column_stats()[2])
    if start == "init":
        model = P.FAModel.init(k, sp, seed=7)
    else:
        c = np.random.default_rng(7).standard_normal((d, k))
        c[~np.isfinite(x).any(axis=0)] = 0.0
        model = P.FAModel(np.ones(d), c, np.zeros(d))
    llks = []
    assert np.all(model.noise == 1.0) and not model.mean.any()
    for _ in range(25):
        model, llk = model.iterate_with_llk(sp, floor)
        llks.append(llk)
    steps = np.diff(llks)
    want = MONOTONE[(start, n, d, k)]
    print("%s (%d, %d, %d): llk %.6e -> %.6e; smallest step %.4e (restatement on the CPU: %.4e); floor active on %d columns" % (
        start, n, d, k, llks[0], llks[-1], steps.min(), want, int((model.noise <= floor).sum())))
    assert np.all(steps >= 0.0) and llks[-1] > llks[0]
    assert abs(steps.min() - want) <= 1e-3 * want  # the same trajectory as the restatement's (its figures are kept to four digits)


def test_trainer_equals_the_dense_trainer(P):
    n, d, k = F.SEAM
    sp = _sparse(P, n, d, k, {})
    ds = sp.to_dense()
    a = P.FATrainer(sp).train(state_size=4, n_iters=5, seed=7, quiet=True)
    b = P.FATrainer(ds).train(state_size=4, n_iters=5, seed=7, quiet=True)
    errs = _dense_model_errors(a, b)
    _show("trainer, sparse vs dense:", errs, TOL)
    assert isinstance(a, P.FAModel) and max(errs.values()) <= TOL, errs


def test_select_state_size_equals_the_dense_trainers(P):
    n, d, k = F.SEAM
    sp = _sparse(P, n, d, k, {})
    got = P.FATrainer(sp).select_state_size([2, 4], fraction=0.15, seed=7, n_iters=5)
    want = P.FATrainer(sp.to_dense()).select_state_size([2, 4], fraction=0.15, seed=7, n_iters=5)
    assert [g[0] for g in got] == [2, 4] and all(isinstance(g[2], P.FAModel) for g in got)
    for (ks, ss, _), (kd, sd, _) in zip(got, want):
        err = abs(ss.mean_llk / sd.mean_llk - 1.0)
        print("select_state_size k=%d: mean_llk %.12g (sparse) %.12g (dense): %.2e (bound %g)" % (ks, ss.mean_llk, sd.mean_llk, err, TOL_OWN))
        assert ss.n_entries == sd.n_entries and err <= TOL_OWN
    folds = P.FATrainer(sp).select_state_size([2], seed=7, n_iters=2, folds=3)
    assert folds[0][1].n_entries == sp.nnz and len(folds[0][2]) == 3


# ------------------------------------------------------------------ 6. errors
def test_errors(P):
    import ctypes as C

    from ppca_rs_amd import _lib

    x, w, (noise, c, mu), _ = F.fa_case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.FAModel(noise, c, mu)
    rng = np.random.default_rng(0)
    ptr = _lib.ptr
    lib, h = _lib.lib(), sp._ctx.handle

    def step(spx, dd, kk, nz):
        cc, mm, out = np.ascontiguousarray(rng.standard_normal((dd, max(kk, 1)))), np.zeros(dd), [np.empty(dd), np.empty((dd, max(kk, 1))), np.empty(dd)]
        return lib.ppca_fa_sparse_em_step(h, spx._sh, dd, kk, ptr(nz), ptr(cc), ptr(mm), None, ptr(out[0]), ptr(out[1]), ptr(out[2]), None)

    assert step(sp, 9, 17, np.ones(9)) == UNSUPPORTED and b"k <= 16" in lib.ppca_last_error()  # k = 17: refused before any launch
    assert step(sp, 10, 3, np.ones(10)) == INVALID  # a mismatched d
    assert step(P.SparseDataset([0], [], [], 9), 9, 3, np.ones(9)) == EMPTY  # an empty dataset
    for bad in (0.0, -1.0, np.nan, np.inf):
        nz = np.ones(9)
        nz[4] = bad
        assert step(sp, 9, 3, nz) == INVALID
    # a non-finite a, b or l: the routine itself (the Python layer answers before it)
    for which in range(3):
        v = [np.ones(9), np.ones(9), np.ones(9)]
        v[which][2] = np.nan
        sums = np.empty((3, 9))
        assert lib.ppca_scale_columns_sparse(h, sp._sh, ptr(v[0]), ptr(v[1]), ptr(v[2]), None, ptr(sums), None) == INVALID
    one = np.ones(9)
    assert lib.ppca_scale_columns_sparse(h, sp._sh, ptr(one), None, None, None, None, None) == INVALID  # no output requested
    with pytest.raises(ValueError, match="finite"):
        sp._scale_columns(np.full(9, np.inf))
    with pytest.raises(P.PPCAError) as err:
        P.FAModel(np.ones(9), rng.standard_normal((9, 17)), np.zeros(9)).llk(sp)
    assert err.value.code == UNSUPPORTED
    with pytest.raises(ValueError, match="output size"):
        P.FAModel(np.ones(10), rng.standard_normal((10, 3)), np.zeros(10)).llks(sp)
    empty = P.SparseDataset([0], [], [], 9)
    with pytest.raises(P.PPCAError) as err:
        model.llk(empty)
    assert err.value.code == EMPTY
    with pytest.raises(ValueError, match="empty"):
        model.iterate(empty)
    train, held = sp.holdout(0.3, 1)
    with pytest.raises(TypeError, match="one of each"):  # one part sparse and one dense
        model.heldout_score(train, held.to_dense())
    with pytest.raises(TypeError, match="one of each"):
        model.heldout_score(train.to_dense(), held)
    with pytest.raises(ValueError, match="block_rows"):  # differing block_rows
        model.heldout_score(train, P.SparseDataset.from_dense(x, block_rows=16))
    with pytest.raises(TypeError):
        model.smooth(sp)
    with pytest.raises(TypeError):
        P.heldout_score(model, train, held)
    assert np.isfinite(model.llk(sp))  # the context is as it was
