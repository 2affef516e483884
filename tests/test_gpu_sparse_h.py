"""PPCA with a known precision per entry on row-compressed data on the GPU: the E-step, one ECM step and
predict of HPPCAModel on a SparseDataset against the row-by-row restatement (tests/hppca_restatement.py), what the design promises bit
for bit, the models it must coincide with, the behaviour of the loop, dirtied recycled memory, and the errors of the C-ABI.

Cases: tests/sparse_h_cases.py::CASES -- the seven shapes of tests/test_gpu_sparse.py at the default tiling, the state-size sweep
k = 1 .. 16 at (150, 300) under block_rows = 64, segment = 8, and the seam shape (300, 300, 4) under four tilings.  A precision per
stored entry, log-uniform in [2^-10, 2^10].  Weights are the case's, its zero weight included.

Bounds, all the project's: TOL = 1e-5 against the restatement with the measures of tests/test_gpu_hppca.py (rows relative to
1 + |value|, sums relative to the sums of their terms' magnitudes; the new model by sparse_fa_cases.model_gaps); DEV = 1e-10 where
both sides are device results; TILE = 1e-11 of the magnitude sums between two tilings.  Every check prints its worst
error before asserting."""
import ctypes as C

import numpy as np
import pytest

import hppca_restatement as R
import sparse_fa_cases as F
import sparse_h_cases as H

pytestmark = pytest.mark.gpu

TOL, DEV, TILE = 1e-5, 1e-10, 1e-11
INVALID, UNSUPPORTED, EMPTY = -1, -3, -4
IDS = [H.case_id(c) for c in H.CASES]
ALL = dict(llks=True, states=True, covs=True, stats=True, scalars=True)
FEW = [(64, 9, 3, {}), (150, 300, 11, {}), (*H.SEAM, H.SEAM_TILINGS[0])]
FEW_IDS = [H.case_id(c) for c in FEW]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _sum_err(got, want, scale):
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())


def _estep_errors(got, e):
    ll, st, cv, ss, sc = got
    return dict(ell=_rel(ll, e["ell"]), z=_rel(st, e["z"]), Sigma=_rel(cv, e["Sigma"]),
                stats=_sum_err(ss, R.packed_stats(e), R.packed_stats(e, "abs")), scalars=_sum_err(sc[:3], e["scalars"], e["scalars_abs"]))


def _show(label, errs, bound=TOL):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % bound)


def _gaps(new, want, d):
    s1, c1, m1 = want
    got = (np.full(d, new.isotropic_noise), new.transform, new.mean)
    return dict(zip(("sigma", "C", "mean"), F.model_gaps(got, (np.full(d, s1), c1, m1))))


def _sparse(P, n, d, k, tiling, weighted=True, ctx=None):
    x, _, w, _, _ = H.case(n, d, k)
    return P.SparseDataset.from_dense(x, w if weighted else None, ctx=ctx, **tiling)


def _model(P, n, d, k, ctx=None):
    s, c, mu = H.case(n, d, k)[3]
    return P.HPPCAModel(s, c, mu, ctx=ctx, row_compressed=d > 1024)


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("n,d,k,tiling", H.CASES, ids=IDS)
def test_against_the_restatement(P, n, d, k, tiling):
    x, p, w, (s, c, mu), pv = H.case(n, d, k)
    e = H.want(n, d, k)
    sp, model = _sparse(P, n, d, k, tiling), _model(P, n, d, k)
    prec = model._sparse_pair(sp, pv)  # (the view, built once for the calls below)
    got = model._estep(sp, prec, **ALL)
    errs = _estep_errors(got, e)
    _show("estep %s:" % H.case_id((n, d, k, tiling)), errs)
    assert max(errs.values()) <= TOL, errs
    ll, st, cv, ss, sc = got
    empty = e["m"] == 0
    assert np.all(ll[empty] == 0) and not st[empty].any() and sc[2] == (~empty).sum() and sc[3] == 0
    assert _rel(cv[empty], np.broadcast_to(np.eye(k), cv[empty].shape)) <= 1e-14
    none = ~np.isfinite(x).any(axis=0)
    cnt = ss[-d:]
    assert not cnt[none].any() and not ss[:d * k].reshape(d, k)[none].any()  # a column without an entry: zeros

    # -- the narrower calls return the same numbers; an array, a SparseDataset of precisions and a view are the same precisions
    assert np.array_equal(model.llks(sp, prec), ll) and np.array_equal(model.llks(sp, pv), ll)
    assert np.array_equal(model.llks(sp, sp.with_values(pv)), ll)
    inf = model.infer(sp, prec)
    assert np.array_equal(inf.states(), st) and np.array_equal(np.array(inf.covariances()), cv)
    assert model.llk(sp, prec) == sc[1]
    only = model._estep(sp, prec, stats=True)[3]
    assert np.array_equal(only, ss)

    # -- one step
    new, llk = model.iterate_with_llk(sp, prec)
    step = _gaps(new, R.mstep(s, c, mu, e), d)
    _show("   iterate:", step)
    assert max(step.values()) <= TOL, step
    want_llk, mag = e["scalars"][1], e["scalars_abs"][1]
    print("   llk %.12e, restatement %.12e: %.1e of the magnitudes (bound %g)" % (llk, want_llk, abs(llk - want_llk) / mag, TOL))
    assert abs(llk - want_llk) <= TOL * mag and abs(llk - sc[1]) <= DEV * mag
    assert new.row_compressed and new.n_parameters == model.n_parameters
    assert np.array_equal(new.transform[none], c[none]) and np.array_equal(new.mean[none], mu[none])
    plain = model.iterate(sp, pv)
    assert plain.isotropic_noise == new.isotropic_noise and np.array_equal(plain.transform, new.transform) and np.array_equal(plain.mean, new.mean)


# ------------------------------------------------------------------ 2. exactness the design promises
def test_bits_do_not_depend_on_tiling_weights_or_grid(P):
    n, d, k = H.SEAM
    x, p, w, _, pv = H.case(n, d, k)
    e = H.want(n, d, k)
    mags = R.packed_stats(e, "abs")
    model = _model(P, n, d, k)
    base = _sparse(P, n, d, k, {})
    ll, st, cv, ss, sc = model._estep(base, pv, **ALL)
    ctx = base._ctx
    worst = 0.0
    try:
        for tiling in ({},) + tuple(H.SEAM_TILINGS):
            for weighted in (True, False):
                sp = _sparse(P, n, d, k, tiling, weighted)
                prec = model._sparse_pair(sp, pv)
                ref = None
                for limit in (0, 1, 3):
                    ctx.set_grid_limit(limit)
                    l2, s2, c2, ss2, sc2 = model._estep(sp, prec, **ALL)
                    assert np.array_equal(l2, ll) and np.array_equal(s2, st) and np.array_equal(c2, cv), (tiling, weighted, limit)
                    ref = (ss2, sc2) if ref is None else ref
                    assert np.array_equal(ss2, ref[0]) and np.array_equal(sc2, ref[1]), (tiling, weighted, limit, "sums under a grid limit")
                if weighted:
                    worst = max(worst, _sum_err(ref[0], ss, mags))
    finally:
        ctx.set_grid_limit(0)
    print("statistics between tilings: %.1e of the magnitude sums (bound %g)" % (worst, TILE))
    assert worst <= TILE
    # a row's outputs do not depend on its position or its neighbours: the second half alone
    half = P.SparseDataset.from_dense(x[150:])
    hl, hs, hc, _, _ = model._estep(half, pv[base.csr()[0][150]:], **ALL)
    assert np.array_equal(hl, ll[150:]) and np.array_equal(hs, st[150:]) and np.array_equal(hc, cv[150:])


@pytest.mark.parametrize("n,d,k,tiling", FEW, ids=FEW_IDS)
def test_doubled_weights_double_the_statistics(P, n, d, k, tiling):
    x, p, w, _, pv = H.case(n, d, k)
    model = _model(P, n, d, k)
    sp = _sparse(P, n, d, k, tiling)
    twice = sp.with_weights(2.0 * w)
    a, b = model._estep(sp, pv, **ALL), model._estep(twice, pv, **ALL)
    assert np.array_equal(b[3], 2.0 * a[3]) and np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1]) and np.array_equal(b[2], a[2])
    assert b[4][0] == 2.0 * a[4][0] and b[4][1] == 2.0 * a[4][1] and b[4][2] == a[4][2]


# ------------------------------------------------------------------ 3. the models it must coincide with
@pytest.mark.parametrize("n,d,k,tiling", FEW, ids=FEW_IDS)
def test_unit_precisions_are_the_gaussian_model(P, n, d, k, tiling):
    model, sp = _model(P, n, d, k), _sparse(P, n, d, k, tiling)
    ll, st, cv, _, _ = model._estep(sp, np.ones(sp.nnz), **ALL)
    g = model.gaussian()
    inf = g.infer(sp)
    errs = dict(ell=_rel(ll, g.llks(sp)), z=_rel(st, inf.states()), Sigma=_rel(cv, np.array(inf.covariances())))
    _show("unit precisions %s:" % H.case_id((n, d, k, tiling)), errs, DEV)
    assert max(errs.values()) <= DEV, errs


@pytest.mark.parametrize("n,d,k,tiling", FEW, ids=FEW_IDS)
def test_column_precisions_are_factor_analysis(P, n, d, k, tiling):
    """p_ij = 1 / psi_j^2 with sigma = 1 is FAModel(psi, C, mean) on the same SparseDataset."""
    x, _, w, (_, c, mu), _ = H.case(n, d, k)
    psi = F.scales(n, d, k)
    sp = _sparse(P, n, d, k, tiling)
    ll, st, cv, _, _ = P.HPPCAModel(1.0, c, mu)._estep(sp, (1.0 / psi ** 2)[sp.csr()[1]], **ALL)
    fa = P.FAModel(psi, c, mu)
    inf = fa.infer(sp)
    errs = dict(ell=_rel(ll, fa.llks(sp)), z=_rel(st, inf.states()), Sigma=_rel(cv, np.array(inf.covariances())))
    _show("column precisions %s:" % H.case_id((n, d, k, tiling)), errs, DEV)
    assert max(errs.values()) <= DEV, errs


DENSE = [c for c in H.CASES if c[1] <= 1024 and (not c[3] or c[:3] == H.SEAM)]


@pytest.mark.parametrize("n,d,k,tiling", DENSE, ids=[H.case_id(c) for c in DENSE])
def test_against_the_dense_path(P, n, d, k, tiling):
    """The dense HPPCAModel on to_dense() with the dense precision array (NaN where nothing is stored)."""
    x, p, w, (s, c, mu), pv = H.case(n, d, k)
    e = H.want(n, d, k)
    model, sp = _model(P, n, d, k), _sparse(P, n, d, k, tiling)
    got = model._estep(sp, pv, **ALL)
    ds = sp.to_dense()
    want = model._estep(ds, p, **ALL)
    mags = R.packed_stats(e, "abs")
    errs = dict(ell=_rel(got[0], want[0]), z=_rel(got[1], want[1]), Sigma=_rel(got[2], want[2]), stats=_sum_err(got[3], want[3], mags),
                scalars=_sum_err(got[4][:3], want[4][:3], e["scalars_abs"]))
    _show("dense path %s:" % H.case_id((n, d, k, tiling)), errs, DEV)
    assert max(errs.values()) <= DEV, errs
    a, b = model.iterate(sp, pv), model.iterate(ds, p)
    step = _gaps(a, (b.isotropic_noise, b.transform, b.mean), d)
    _show("   iterate:", step, DEV)
    assert max(step.values()) <= DEV, step


# ------------------------------------------------------------------ 4. the use
@pytest.mark.parametrize("n,d,k", H.MONOTONE, ids=["%dx%dx%d" % s for s in H.MONOTONE])
def test_llk_never_decreases(P, n, d, k):
    _, _, _, _, pv = H.case(n, d, k)
    sp, model = _sparse(P, n, d, k, H.SWEEP_TILING), _model(P, n, d, k)
    prec = model._sparse_pair(sp, pv)
    llks = []
    for _ in range(10):
        model, llk = model.iterate_with_llk(sp, prec)
        llks.append(llk)
    llks.append(model.llk(sp, prec))
    steps = np.diff(llks)
    print("llk %dx%dx%d: %.6e -> %.6e, smallest step %.2e" % (n, d, k, llks[0], llks[-1], steps.min()))
    assert np.all(steps >= -1e-9 * np.abs(llks[:-1])) and llks[-1] > llks[0]


def test_trainer(P):
    n, d, k = H.SEAM
    _, _, _, _, pv = H.case(n, d, k)
    sp = _sparse(P, n, d, k, H.SWEEP_TILING)
    model, metrics = P.HPPCATrainer(sp, pv).train(state_size=k, n_iters=4, seed=3)
    assert isinstance(model, P.HPPCAModel) and model.row_compressed and len(metrics) == 4
    gram = model.transform.T @ model.transform  # canonical: orthogonal columns, in descending length
    off = np.abs(gram - np.diag(np.diag(gram))).max() / np.diag(gram).max()
    print("trainer: off-diagonal of C^T C %.1e of its largest diagonal entry" % off)
    assert off <= 1e-12 and np.all(np.diff(np.diag(gram)) <= 0)
    start = P.HPPCAModel.init(k, sp, seed=3)
    by_hand = start
    llks = []
    for _ in range(4):
        by_hand, llk = by_hand.iterate_with_llk(sp, sp.with_values(pv))
        llks.append(llk)
    assert [m.llk for m in metrics] == [v / n for v in llks] and model.isotropic_noise  # (TrainMetrics.llk is per sample) == by_hand.isotropic_noise
    assert np.array_equal(model.transform, by_hand.to_canonical().transform) and np.array_equal(model.mean, by_hand.mean)
    assert all(np.isfinite([m.aic, m.bic]).all() for m in metrics)


def test_the_sparse_two_noise_level_case(P):
    """Thirty steps with the true precisions end below the midpoint of the restatement's two angles (4.04 and 26.78 degrees,
    tests/test_sparse_h_host.py), thirty PPCAModel steps on the same data above it."""
    x, p, c_true, start = H.hetero_case()
    sp = P.SparseDataset.from_dense(x)
    pv = p[np.isfinite(x)]
    mid = 0.5 * sum(H.HETERO_ANGLES)
    h = P.HPPCAModel(1.0, start, np.zeros(x.shape[1]))
    prec = h._sparse_pair(sp, pv)
    g = h.gaussian()
    for _ in range(H.HETERO["iters"]):
        h = h.iterate(sp, prec)
        g = g.iterate(sp)
    ah, ag = R.subspace_angle(h.transform, c_true), R.subspace_angle(g.transform, c_true)
    print("true precisions: %.3f degrees (sigma %.3f); PPCAModel: %.3f degrees (sigma %.3f); midpoint %.2f" %
          (ah, h.isotropic_noise, ag, g.isotropic_noise, mid))
    assert ah < mid < ag


# ------------------------------------------------------------------ 5. predict
@pytest.mark.parametrize("n,d,k,tiling", FEW + [(40, 70000, 3, {})], ids=FEW_IDS + ["40x70000x3"])
def test_predict(P, n, d, k, tiling):
    x, p, w, (s, c, mu), pv = H.case(n, d, k)
    e = H.want(n, d, k)
    sp, model = _sparse(P, n, d, k, tiling), _model(P, n, d, k)
    cols = np.unique(np.minimum(np.array([0, 3, 5, 7, d // 2, d - 1]), d - 1)).astype(np.int32)
    indptr = np.arange(n + 1, dtype=np.int64) * cols.size
    indices = np.tile(cols, n)
    mean, var = model.predict(sp, pv, (indptr, indices))
    rows = np.repeat(np.arange(n), cols.size)
    want_mean = mu[indices] + np.einsum("ek,ek->e", c[indices], e["z"][rows])
    want_var = np.einsum("ek,ekl,el->e", c[indices], e["Sigma"][rows], c[indices]) + s * s
    errs = dict(mean=_rel(mean, want_mean), var=_rel(var, want_var))
    _show("predict %s:" % H.case_id((n, d, k, tiling)), errs)
    assert max(errs.values()) <= TOL, errs
    none = np.flatnonzero(e["m"] == 0)
    assert none.size
    for i in none:  # a row without a stored entry: the prior predictive
        sl = slice(indptr[i], indptr[i + 1])
        assert np.array_equal(mean[sl], mu[cols]) and _rel(var[sl], (c[cols] ** 2).sum(axis=1) + s * s) <= 1e-14
    m2, v2 = model.predict(sp, sp.with_values(pv), sp)  # a SparseDataset as the query: its pattern
    assert m2.shape == (sp.nnz,) and np.all(v2 > 0)


# ------------------------------------------------------------------ 6. dirtied recycled memory
def _four_entry_points(P, ctx, n, d, k, tiling):
    """ppca_h_sparse_precisions, _estep, _em_step and _predict on datasets, a view and a model made and released inside."""
    x, _, w, (s, c, mu), pv = H.case(n, d, k)
    sp = P.SparseDataset.from_dense(x, w, ctx=ctx, **tiling)
    model = P.HPPCAModel(s, c, mu, ctx=ctx)
    prec = model._sparse_pair(sp, pv)
    ll, st, cv, ss, sc = model._estep(sp, prec, **ALL)
    new, llk = model.iterate_with_llk(sp, prec)
    mean, var = model.predict(sp, prec, sp)
    # the view's own two buffers, read back through the passes that consume them one at a time: the row side (llks above) and the
    # column side (the statistics above)
    return dict(ll=ll, st=st, cv=cv, ss=ss, sc=sc, sigma=np.float64(new.isotropic_noise), C=new.transform, mu=new.mean,
                llk=np.float64(llk), mean=mean, var=var)


@pytest.mark.parametrize("n,d,k,tiling", [(150, 300, 3, H.SWEEP_TILING), (150, 300, 16, H.SWEEP_TILING)], ids=["k3", "k16"])
def test_dirtied_memory(P, n, d, k, tiling):
    """Each of the four entry points on a private context: twice as it comes, then after dirty_scratch(0xFF) (every double a NaN) and
    after (0x3F) -- all four results bit for bit equal, and the 0xFF run also matches the restatement."""
    from ppca_rs_amd import _lib

    ctx = _lib.Context()
    try:
        runs = [_four_entry_points(P, ctx, n, d, k, tiling), _four_entry_points(P, ctx, n, d, k, tiling)]
        for fill in (0xFF, 0x3F):
            blocks, nbytes = ctx.dirty_scratch(fill)
            assert blocks >= 1 and nbytes >= 8 * H.case(n, d, k)[4].size, (blocks, nbytes)
            runs.append(_four_entry_points(P, ctx, n, d, k, tiling))
    finally:
        ctx.trim()
    for i, r in enumerate(runs[1:], 1):
        bad = [key for key in runs[0] if _bytes(r[key]) != _bytes(runs[0][key])]
        assert not bad, ("run %d differs from run 0 in" % i, bad)
    e = H.want(n, d, k)
    r = runs[2]
    errs = _estep_errors((r["ll"], r["st"], r["cv"], r["ss"], r["sc"]), e)
    s, c, mu = H.case(n, d, k)[3]
    want = R.mstep(s, c, mu, e)
    errs.update(dict(zip(("sigma", "C", "mean"), F.model_gaps((np.full(d, r["sigma"]), r["C"], r["mu"]), (np.full(d, want[0]),) + want[1:]))))
    _show("after the 0xFF fill, k = %d:" % k, errs)
    assert max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ 7. the errors of the C-ABI
def test_errors(P, hiplib):
    from ppca_rs_amd._lib import ptr

    n, d, k = 64, 9, 3
    x, _, w, (s, c, mu), pv = H.case(n, d, k)
    sp, model = _sparse(P, n, d, k, {}), _model(P, n, d, k)
    ctx = sp._ctx
    prec = model._sparse_pair(sp, pv)
    dev = model.gaussian()._device(ctx).h
    out = np.empty(n)
    # a view of another dataset (the same pattern, uploaded on its own) is refused: no pattern is compared on the device
    twin = _sparse(P, n, d, k, {})
    assert hiplib.ppca_h_sparse_estep(dev, ctx.handle, twin._sh, prec._handle, ptr(out), None, None, None, None) == INVALID
    assert b"not a view" in hiplib.ppca_last_error()
    assert hiplib.ppca_h_sparse_estep(dev, ctx.handle, sp._sh, sp._sh, ptr(out), None, None, None, None) == INVALID  # not a view at all
    with pytest.raises(ValueError, match="another pattern"):
        model.llks(twin, prec)
    # ... but a dataset that shares the pattern on the device takes it
    assert np.array_equal(model.llks(sp.with_weights(np.ones(n)), prec), model.llks(sp, prec))
    assert hiplib.ppca_h_sparse_estep(dev, ctx.handle, sp._sh, prec._handle, None, None, None, None, None) == INVALID  # no output
    # a bad precision, in C
    bad = pv.copy()
    for v in (0.0, -1.0, np.nan, np.inf):
        bad[5] = v
        h = C.c_void_p()
        assert hiplib.ppca_h_sparse_precisions(ptr(bad), ctx.handle, sp._sh, C.byref(h)) == INVALID and not h
    # state sizes beyond 16, and 0: before any launch
    big_model, zero_model, other_model = (P.PPCAModel(s, np.ones((d, 17)), mu), P.PPCAModel(s, np.zeros((d, 0)), mu),
                                          P.PPCAModel(s, np.ones((d + 1, k)), np.zeros(d + 1)))  # (alive while their handles are used)
    big = big_model._device(ctx).h
    assert hiplib.ppca_h_sparse_estep(big, ctx.handle, sp._sh, prec._handle, ptr(out), None, None, None, None) == UNSUPPORTED
    zero = zero_model._device(ctx).h
    assert hiplib.ppca_h_sparse_estep(zero, ctx.handle, sp._sh, prec._handle, ptr(out), None, None, None, None) == UNSUPPORTED
    s1, c17, m1 = C.c_double(0.0), np.ones((d, 17)), np.empty(d)
    assert hiplib.ppca_h_sparse_em_step(d, 17, C.c_double(s), ptr(c17), ptr(mu), ctx.handle, sp._sh, prec._handle, C.byref(s1), ptr(c17.copy()),
                                        ptr(m1), None) == UNSUPPORTED
    # another output size
    other = other_model._device(ctx).h
    assert hiplib.ppca_h_sparse_estep(other, ctx.handle, sp._sh, prec._handle, ptr(out), None, None, None, None) == INVALID
    # an empty dataset: a view of it can be made, every pass answers PPCA_ERR_EMPTY
    empty = P.SparseDataset([0], [], [], d)
    h = C.c_void_p()
    assert hiplib.ppca_h_sparse_precisions(None, ctx.handle, empty._sh, C.byref(h)) == 0 and h
    try:
        assert hiplib.ppca_h_sparse_estep(dev, ctx.handle, empty._sh, h, ptr(out), None, None, None, None) == EMPTY
        assert hiplib.ppca_h_sparse_predict(dev, ctx.handle, empty._sh, h, None, None, None, None) == EMPTY
    finally:
        hiplib.ppca_sparse_free(h)
    # ppca_em_last_llk keeps reporting the last plain step
    g = model.gaussian()
    _, plain_llk = g.iterate_with_llk(sp)
    model.iterate(sp, prec)
    last = C.c_double(0.0)
    assert hiplib.ppca_em_last_llk(ctx.handle, C.byref(last)) == 0 and last.value == plain_llk
    with pytest.raises(TypeError):
        model.predict(sp.to_dense(), pv, (sp.csr()[0], sp.csr()[1]))
