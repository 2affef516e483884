"""Student-t PPCA on row-compressed data on the GPU: the E-step and one ECM step of TPPCAModel on a
SparseDataset against the row-by-row restatement (tests/tppca_restatement.py) and against the library's dense path, what the design
promises bit for bit, the behaviour of the loop, and the errors of the C-ABI.

Cases: tests/sparse_t_cases.py::CASES -- the seven shapes of tests/test_gpu_sparse.py at the default tiling with nu in {0.7, 4, 200},
the state-size sweep k = 1 .. 16 at (150, 300) under block_rows = 64, segment = 8, and the seam shape (300, 300, 4) under four tilings.
Weights are the case's, its zero weight included.

Bounds: those of tests/test_gpu_robust.py.  TOL = 1e-5, the project's GPU parity bound: delta, u, ell relative to 1 + |value|; V, A,
T, sq and the scalars relative to the sum of their terms' magnitudes (the restatement's `abs`); sigma relative, C against max |C|,
mean_j against max(|mean_j|, sigma).  The returned llk against the restatement's at 1e-9 relative, the estimated nu to nine digits.
Every check prints its worst error before asserting."""
import ctypes as C

import numpy as np
import pytest

import sparse_t_cases as T
import tppca_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
INVALID, UNSUPPORTED, EMPTY = -1, -3, -4
IDS = [T.case_id(c) for c in T.CASES]
DENSE = [c for c in T.CASES if c[1] <= 1024 and c[3] == T.NU]
ALL = dict(scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _sum_err(got, want, scale):
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())


def _split(cs, d, k):
    return cs[:d * k].reshape(d, k), cs[d * k:d * k + d], cs[d * k + d:d * k + 2 * d], cs[d * k + 2 * d:]


def _estep_errors(got, e, d, k):
    _, cs, u, delta, ell, sc = got
    V, A, T_, sq = _split(cs, d, k)
    return dict(delta=_rel(delta, e["delta"]), u=_rel(u, e["u"]), ell=_rel(ell, e["ell"]), V=_sum_err(V, e["V"], e["abs"]["V"]),
                A=_sum_err(A, e["A"], e["abs"]["A"]), T=_sum_err(T_, e["T"], e["abs"]["T"]), sq=_sum_err(sq, e["sq"], e["abs"]["sq"]),
                scalars=_sum_err(sc, e["scalars"], e["scalars_abs"]))


def _model_errors(new, want):
    s1, c1, m1 = want
    return dict(sigma=abs(new.isotropic_noise / s1 - 1), C=float(np.abs(new.transform - c1).max() / np.abs(c1).max()),
                mean=float((np.abs(new.mean - m1) / np.maximum(np.abs(m1), s1)).max()))


def _show(label, errs, bound=TOL):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % bound)


def _sparse(P, n, d, k, tiling, weighted=True):
    x, w, _ = T.case(n, d, k)
    return P.SparseDataset.from_dense(x, w if weighted else None, **tiling)


def _model(P, n, d, k, nu):
    _, _, (s, c, mu) = T.case(n, d, k)
    return P.TPPCAModel(s, c, mu, nu, row_compressed=d > 1024)


def _stats_raw(P, model, sp):
    from ppca_rs_amd._lib import check, lib, ptr

    out = np.empty(int(lib().ppca_stats_len(model.output_size, model.state_size)))
    check(lib().ppca_sparse_stats_raw(sp._ctx.handle, sp._sh, model._device(sp._ctx).h, ptr(out)))
    return out


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("n,d,k,nu,tiling", T.CASES, ids=IDS)
def test_against_the_restatement(P, n, d, k, nu, tiling):
    x, w, (s, c, mu) = T.case(n, d, k)
    e = T.want(n, d, k, nu)
    sp = _sparse(P, n, d, k, tiling)
    model = _model(P, n, d, k, nu)
    got = model._estep(sp, **ALL)
    errs = _estep_errors(got, e, d, k)
    _show("estep %s:" % T.case_id((n, d, k, nu, tiling)), errs)
    assert max(errs.values()) <= TOL, errs
    view, cs, u, delta, ell, sc = got
    empty = e["m"] == 0
    assert np.all(delta[empty] == 0) and np.all(u[empty] == 1) and np.all(ell[empty] == 0)
    assert np.all(u <= (nu + e["m"]) / nu * (1 + 1e-15)) and np.all(u > 0)
    V, A, T_, sq = _split(cs, d, k)
    none = ~np.isfinite(x).any(axis=0)
    assert not V[none].any() and not A[none].any() and not T_[none].any() and not sq[none].any()  # a column without an entry: zeros

    # -- the view: made on the device, fetched on demand; its CSR values from the RETURNED u, bit for bit
    indptr, indices, values = sp.csr()
    assert isinstance(view, P.SparseDataset) and view._handle is not None and view._vals is None
    vp, vi, vv = view.csr()
    rows = np.repeat(np.arange(n), np.diff(indptr))
    assert np.array_equal(vv, np.sqrt(u)[rows] * (values - mu[indices]))  # fl(fl(sqrt u) fl(x - mean))
    assert np.array_equal(vp, indptr) and np.array_equal(vi, indices) and np.array_equal(view.weights(), w)
    # -- its index-order copy: the statistics pass on the view against the same pass on a dataset built from the view's CSR
    g0 = P.PPCAModel(s, c, np.zeros(d))
    fresh = P.SparseDataset(vp, vi, vv, d, w, **tiling)
    assert np.array_equal(_stats_raw(P, g0, view), _stats_raw(P, g0, fresh))

    # -- the narrower calls return the same numbers
    assert np.array_equal(model.llks(sp), ell) and np.array_equal(model.row_weights(sp), u)
    dm, m = model.mahalanobis(sp)
    assert np.array_equal(dm, delta) and np.array_equal(m, e["m"])
    nothing, cs2, u2, _, _, sc2 = model._estep(sp, col_sums=True, u=True, scalars=True)
    assert nothing is None and np.array_equal(cs2, cs) and np.array_equal(u2, u) and np.array_equal(sc2, sc)
    only = model._estep(sp, scaled=True)[0]  # the view alone: the same bits
    assert np.array_equal(only.csr()[2], vv)
    assert model.llk(sp) == sc[1]
    z = model.infer(sp).states()
    assert np.array_equal(z, model.gaussian().infer(sp).states()) and _rel(z, e["z"]) <= TOL

    # -- one step
    new, llk = model.iterate_with_llk(sp)
    step = _model_errors(new, R.mstep(s, c, mu, e))
    _show("   iterate:", step)
    assert max(step.values()) <= TOL, step
    want_llk = e["scalars"][1]
    print("   llk %.12e, restatement %.12e: %.1e (bound 1e-9)" % (llk, want_llk, abs(llk / want_llk - 1)))
    assert llk == model.llk(sp)  # bit for bit
    assert abs(llk / want_llk - 1) <= 1e-9
    assert new.dof == nu and new.n_parameters == model.n_parameters and new.row_compressed
    assert np.array_equal(new.transform[none], c[none]) and np.array_equal(new.mean[none], mu[none])
    plain = model.iterate(sp)
    assert plain.isotropic_noise == new.isotropic_noise and np.array_equal(plain.transform, new.transform) and np.array_equal(plain.mean, new.mean)
    est = model.iterate(sp, estimate_dof=True)
    want_nu = R.dof_root(e["scalars"][2] / e["scalars"][0])
    print("   nu %.9g, restatement %.9g" % (est.dof, want_nu))
    assert abs(est.dof / want_nu - 1) <= 1e-9 and np.array_equal(est.transform, new.transform)
    assert est.n_parameters == model.n_parameters + 1


def test_predict_is_the_gaussian_models(P):
    n, d, k = 64, 9, 3
    sp = _sparse(P, n, d, k, {})
    model = _model(P, n, d, k, T.NU)
    q = (sp.csr()[0], sp.csr()[1])
    (m1, v1), (m0, v0) = model.predict(sp, q), model.gaussian().predict(sp, q)
    assert np.array_equal(m1, m0) and np.array_equal(v1, v0) and m1.shape == (sp.nnz,)
    with pytest.raises(TypeError):
        model.predict(sp.to_dense(), q)


def test_on_an_empty_dataset(P):
    model = P.TPPCAModel(1.0, np.ones((5, 2)), np.zeros(5), 4.0)
    view, cs, u, delta, ell, sc = model._estep(P.SparseDataset([0], [], [], 5), **ALL)
    assert len(view) == 0 and view.nnz == 0 and view.csr()[2].shape == (0,)
    assert np.array_equal(cs, np.zeros(25)) and u.shape == (0,) and np.array_equal(sc, np.zeros(4))
    rowless = P.SparseDataset(np.zeros(4, dtype=np.int64), [], [], 5)  # rows, but no entry
    view, cs, u, delta, ell, sc = model._estep(rowless, **ALL)
    assert view.nnz == 0 and not cs.any() and np.all(u == 1) and not delta.any() and not ell.any()
    g0 = R.tables(0, 4.0)[1][0]
    assert sc[0] == 3 and sc[1] == 0 and sc[3] == 0 and abs(sc[2] - 3 * (g0 - 1.0)) <= 1e-12


# ------------------------------------------------------------------ 2. exactness the design promises
def test_bits_do_not_depend_on_tiling_weights_or_grid(P):
    n, d, k = T.SEAM
    model = _model(P, n, d, k, T.NU)
    base = _sparse(P, n, d, k, {})
    view, _, u, delta, ell, _ = model._estep(base, **ALL)
    values = view.csr()[2]
    ctx = base._ctx
    try:
        for tiling in ({},) + tuple(T.SEAM_TILINGS):
            for weighted in (True, False):
                sp = _sparse(P, n, d, k, tiling, weighted)
                ref = None
                for limit in (0, 1, 3):
                    ctx.set_grid_limit(limit)
                    v, cs, ug, dg, lg, sc = model._estep(sp, **ALL)
                    assert np.array_equal(ug, u) and np.array_equal(dg, delta) and np.array_equal(lg, ell), (tiling, weighted, limit)
                    assert np.array_equal(v.csr()[2], values), (tiling, weighted, limit)
                    ref = (cs, sc) if ref is None else ref
                    assert np.array_equal(cs, ref[0]) and np.array_equal(sc, ref[1]), (tiling, weighted, limit, "sums under a grid limit")
    finally:
        ctx.set_grid_limit(0)
    # a row's outputs do not depend on its position or its neighbours: the second half alone
    x, _, _ = T.case(n, d, k)
    half = P.SparseDataset.from_dense(x[150:])
    hv, _, hu, hd, hl, _ = model._estep(half, **ALL)
    assert np.array_equal(hu, u[150:]) and np.array_equal(hd, delta[150:]) and np.array_equal(hl, ell[150:])
    assert np.array_equal(hv.csr()[2], values[base.csr()[0][150]:])


EXACT = [(64, 9, 3, {}), (150, 300, 11, {}), (*T.SEAM, T.SEAM_TILINGS[0])]


@pytest.mark.parametrize("n,d,k,tiling", EXACT, ids=["%dx%dx%d" % c[:3] for c in EXACT])
@pytest.mark.parametrize("p", [10, -10])
def test_power_of_two_units_are_exact(P, n, d, k, tiling, p):
    """The data, the mean, C and sigma multiplied by 2^p: u and delta keep their bits and the view is scaled by exactly 2^p."""
    x, w, (s, c, mu) = T.case(n, d, k)
    f = 2.0 ** p
    sp, sps = P.SparseDataset.from_dense(x, w, **tiling), P.SparseDataset.from_dense(x * f, w, **tiling)
    m, ms = P.TPPCAModel(s, c, mu, T.NU), P.TPPCAModel(s * f, c * f, mu * f, T.NU)
    (va, _, ua, da, _, _), (vb, _, ub, db, _, _) = m._estep(sp, **ALL), ms._estep(sps, **ALL)
    assert np.array_equal(ua, ub) and np.array_equal(da, db)
    assert np.array_equal(vb.csr()[2], va.csr()[2] * f)


# ------------------------------------------------------------------ 3. against the dense path
@pytest.mark.parametrize("n,d,k,nu,tiling", DENSE, ids=[T.case_id(c) for c in DENSE])
def test_against_the_dense_path(P, n, d, k, nu, tiling):
    x, w, (s, c, mu) = T.case(n, d, k)
    sp = _sparse(P, n, d, k, tiling)
    ds = sp.to_dense()
    model = P.TPPCAModel(s, c, mu, nu)
    (_, _, us, dls, ls, _), (_, _, ud, dld, ld, _) = model._estep(sp, u=True, maha=True, llks=True), model._estep(ds, u=True, maha=True, llks=True)
    errs = dict(u=_rel(us, ud), delta=_rel(dls, dld), ell=_rel(ls, ld))
    (a, llk_s), (b, llk_d) = model.iterate_with_llk(sp), model.iterate_with_llk(ds)
    errs.update(_model_errors(a, (b.isotropic_noise, b.transform, b.mean)))
    errs["llk"] = abs(llk_s - llk_d) / max(float(np.abs(w * ld).sum()), 1.0)
    _show("dense path %s:" % T.case_id((n, d, k, nu, tiling)), errs)
    assert max(errs.values()) <= TOL, errs
    assert a.row_compressed and not b.row_compressed


# ------------------------------------------------------------------ 4. behaviour
# the smallest of the 25 steps of tppca_restatement.iterate from the case's scoring model at nu = 4, computed on the CPU: (nu fixed,
# estimate_dof); |llk| <= 1e5 there, so a step's rounding is some 1e-10 and no step is near the bound
RESTATEMENT_STEPS = {(300, 300, 4): (0.194, 0.269), (150, 300, 11): (54.9, 69.3), (64, 9, 3): (0.087, 0.081)}


@pytest.mark.parametrize("estimate", [False, True], ids=["nu-fixed", "nu-estimated"])
@pytest.mark.parametrize("n,d,k", T.MONOTONE, ids=["%dx%dx%d" % c for c in T.MONOTONE])
def test_llk_never_decreases(P, n, d, k, estimate):
    sp = _sparse(P, n, d, k, {})
    model = _model(P, n, d, k, T.NU)
    llks = []
    for _ in range(25):
        model, llk = model.iterate_with_llk(sp, estimate_dof=estimate)
        llks.append(llk)
    llks = np.array(llks)
    steps = np.diff(llks)
    print("(%d, %d, %d) %s: llk %.6e -> %.6e; smallest step %+.3e (restatement on the CPU: %+.3g); sigma %.4f nu %.3f" % (
        n, d, k, "estimate_dof" if estimate else "nu fixed", llks[0], llks[-1], steps.min(), RESTATEMENT_STEPS[(n, d, k)][int(estimate)],
        model.isotropic_noise, model.dof))
    assert np.all(steps >= -1e-9 * np.abs(llks[1:])), steps.min()


def test_contaminated_case(P):
    x, c_true, bad, c0 = T.contaminated()
    sp = P.SparseDataset.from_dense(x)
    d = x.shape[1]
    assert np.isfinite(x).sum(axis=1).min() == 3
    t, g = P.TPPCAModel(1.0, c0, np.zeros(d), 4.0), P.PPCAModel(1.0, c0, np.zeros(d))
    for _ in range(30):
        t, g = t.iterate(sp), g.iterate(sp)
    at, ag = R.subspace_angle(t.transform, c_true), R.subspace_angle(g.transform, c_true)
    u = t.row_weights(sp)
    print("t: %.2f degrees, sigma %.3f; PPCAModel.iterate: %.2f degrees, sigma %.3f; median u contaminated %.4f clean %.3f"
          % (at, t.isotropic_noise, ag, g.isotropic_noise, np.median(u[bad]), np.median(u[~bad])))
    assert at < 8.0 and 0.40 < t.isotropic_noise < 0.55
    assert np.median(u[bad]) < 0.05 and np.median(u[~bad]) > 0.6
    assert ag > 30.0


def test_trainer_equals_the_dense_trainer(P):
    n, d, k = T.SEAM
    sp = _sparse(P, n, d, k, {})
    a = P.TPPCATrainer(sp).train(state_size=4, n_iters=5, seed=7, quiet=True)
    b = P.TPPCATrainer(sp.to_dense()).train(state_size=4, n_iters=5, seed=7, quiet=True)
    errs = _model_errors(a, (b.isotropic_noise, b.transform, b.mean))
    _show("trainer, sparse vs dense:", errs)
    assert isinstance(a, P.TPPCAModel) and a.row_compressed and a.dof == b.dof and max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ 5. errors through the C-ABI
def test_errors(P):
    from ppca_rs_amd import _lib

    x, w, (s, c, mu) = T.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    ctx = sp._ctx
    lib, h, ptr = _lib.lib(), sp._ctx.handle, _lib.ptr
    rng = np.random.default_rng(0)
    out = np.empty(64)

    def estep(spx, model, dof, u=out):
        return lib.ppca_t_sparse_estep(h, spx._sh, model._device(ctx).h, dof, None, None, ptr(u), None, None, None)

    def step(spx, dd, kk, dof):
        cc, mm = np.ascontiguousarray(rng.standard_normal((dd, kk))), np.zeros(dd)
        s1, c1, m1 = C.c_double(0.0), np.empty((dd, kk)), np.empty(dd)
        return lib.ppca_t_sparse_em_step(h, spx._sh, dd, kk, 1.0, ptr(cc), ptr(mm), dof, C.byref(s1), ptr(c1), ptr(m1), None, None)

    good = P.PPCAModel(s, c, mu)
    ctx.enable_timing(True)
    try:  # k = 17: refused with nothing launched
        ctx.kernel_time(reset=True)
        assert estep(sp, P.PPCAModel(1.0, np.ones((9, 17)), np.zeros(9)), 4.0) == UNSUPPORTED and b"k <= 16" in lib.ppca_last_error()
        assert step(sp, 9, 17, 4.0) == UNSUPPORTED and b"k <= 16" in lib.ppca_last_error()
        with pytest.raises(_lib.PPCAError):
            _lib.check(step(sp, 9, 17, 4.0))
        assert ctx.kernel_time(reset=True)[1] == 0
    finally:
        ctx.enable_timing(False)
    assert estep(sp, P.PPCAModel(1.0, np.ones((10, 3)), np.zeros(10)), 4.0) == INVALID  # another d
    assert step(sp, 10, 3, 4.0) == INVALID
    assert estep(sp, good, 4.0, None) == INVALID and b"no output" in lib.ppca_last_error()  # all outputs null
    for dof in (0.0, -1.0, np.nan, np.inf):
        assert estep(sp, good, dof) == INVALID and step(sp, 9, 3, dof) == INVALID
    empty = P.SparseDataset([0], [], [], 9)
    assert step(empty, 9, 3, 4.0) == EMPTY
    assert estep(empty, good, 4.0) == 0  # the E-step of an empty dataset gives zeros
    with pytest.raises(P.PPCAError) as err:  # a flagged model on a dense Dataset beyond d = 1024: the library's own answer
        P.TPPCAModel(1.0, np.ones((1025, 2)), np.zeros(1025), 4.0, row_compressed=True).llks(P.Dataset(np.zeros((4, 1025))))
    assert err.value.code == UNSUPPORTED
    assert np.isfinite(P.TPPCAModel(s, c, mu, 4.0).llk(sp))  # the context is as it was
