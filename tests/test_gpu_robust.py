"""Student-t PPCA on the GPU (TPPCAModel): the streaming sweep and the ECM step against the row-by-row
restatement (tests/tppca_restatement.py), what the sweep promises exactly (the scaled rows bit for bit, sums that depend on the grid
only in their last bits, per-row outputs that do not depend on the grid or on a slice), and the model's properties.

Tolerance: the project's GPU parity tolerance, 1e-5 (TOL of tests/test_gpu_factor_noise.py): per row relative to 1 + |value|, sums
relative to the sum of their terms' magnitudes; sigma relative, C against max |C|, mean_j against max(|mean_j|, sigma).  Each parity
check prints its worst error before asserting."""
import ctypes as C
import functools

import numpy as np
import pytest

import mask_patterns as MP
import state_size_cases as S
import tppca_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@functools.lru_cache(maxsize=None)
def _case(n, d, k):
    x, w, model = R.masked_case(n, d, k, 1000 + 31 * n + 7 * d + k)
    for a in (x, w) + model[1:]:
        a.setflags(write=False)
    return x, w, model


@functools.lru_cache(maxsize=None)
def _want(n, d, k, nu):
    x, w, (s, c, mu) = _case(n, d, k)
    return R.estep(x, w, s, c, mu, nu)


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _sum_err(got, want, scale):
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())


def _split(cs, d, k):
    return cs[:d * k].reshape(d, k), cs[d * k:d * k + d], cs[d * k + d:d * k + 2 * d], cs[d * k + 2 * d:]


def _estep_errors(got, e, d, k):
    y, cs, u, delta, ell, sc = got
    V, A, T, sq = _split(cs, d, k)
    errs = dict(delta=_rel(delta, e["delta"]), u=_rel(u, e["u"]), ell=_rel(ell, e["ell"]), V=_sum_err(V, e["V"], e["abs"]["V"]),
                A=_sum_err(A, e["A"], e["abs"]["A"]), T=_sum_err(T, e["T"], e["abs"]["T"]), sq=_sum_err(sq, e["sq"], e["abs"]["sq"]),
                scalars=_sum_err(sc, e["scalars"], e["scalars_abs"]))
    return errs


SHAPES = [(1, 1, 1), (3, 5, 2), (65, 17, 3), (257, 64, 10), (600, 256, 10), (300, 257, 4), (2000, 200, 16), (300, 512, 16), (200, 1024, 16)]


@pytest.mark.parametrize("n,d,k", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_estep_against_restatement(P, n, d, k):
    _check_estep(P, _case(n, d, k), _want(n, d, k, 4.0), 4.0)


def _check_estep(P, case, e, nu):
    x, w, (s, c, mu) = case
    (n, d), k = x.shape, c.shape[1]
    ds = P.Dataset(x, w)
    model = P.TPPCAModel(s, c, mu, nu)
    got = model._estep(ds, scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True)
    errs = _estep_errors(got, e, d, k)
    print("estep %dx%dx%d" % (n, d, k), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs
    y, cs, u, delta, ell, sc = got
    empty = e["m"] == 0
    assert np.all(delta[empty] == 0) and np.all(u[empty] == 1) and np.all(ell[empty] == 0)
    assert np.all(u <= (nu + e["m"]) / nu * (1 + 1e-15)) and np.all(u > 0)

    # -- what needs no tolerance budget from the posterior pass: recomputed from the RETURNED u
    obs = np.isfinite(x)
    xt = x - mu
    yy = y.numpy()
    assert np.array_equal(yy[obs], (np.sqrt(u)[:, None] * xt)[obs]) and np.isnan(yy[~obs]).all()  # fl(fl(sqrt u) fl(x - mean))
    assert np.array_equal(y.weights(), w)
    V, A, T, sq = _split(cs, d, k)
    wu = (w * u)[:, None] * obs
    xz = np.where(obs, xt, 0.0)
    ex = dict(A=_sum_err(A, (wu * xz).sum(0), (wu * np.abs(xz)).sum(0)), T=_sum_err(T, wu.sum(0), wu.sum(0)),
              sq=_sum_err(sq, (wu * xz * xz).sum(0), (wu * xz * xz).sum(0)))
    z = model.infer(ds).states()
    ex["V"] = _sum_err(V, wu.T @ z, wu.T @ np.abs(z))
    print("   from the returned u:", " ".join("%s %.1e" % kv for kv in ex.items()), "(bounds 1e-11, V 1e-10)")
    assert max(ex["A"], ex["T"], ex["sq"]) <= 1e-11 and ex["V"] <= 1e-10, ex
    dm, m = model.mahalanobis(ds)
    assert np.array_equal(dm, delta) and np.array_equal(m, e["m"])

    # -- the narrower calls return the same numbers
    assert np.array_equal(model.llks(ds), ell) and np.array_equal(model.row_weights(ds), u)
    none, cs2, u2, _, _, sc2 = model._estep(ds, col_sums=True, u=True, scalars=True)
    assert none is None and np.array_equal(cs2, cs) and np.array_equal(u2, u) and np.array_equal(sc2, sc)
    assert model.llk(ds) == sc[1]

    # -- under a capped grid: per-row outputs and the scaled rows bit for bit, the sums to 1e-11
    ctx = ds._ctx
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            yg, csg, ug, dg, lg_, scg = model._estep(ds, scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True)
            assert np.array_equal(ug, u) and np.array_equal(dg, delta) and np.array_equal(lg_, ell)
            assert np.array_equal(yg.numpy(), yy, equal_nan=True)
            scale = np.concatenate([(wu.T @ np.abs(z)).ravel(), (wu * np.abs(xz)).sum(0), wu.sum(0), (wu * xz * xz).sum(0)])
            assert _sum_err(csg, cs, scale) <= 1e-11 and _sum_err(scg, sc, e["scalars_abs"]) <= 1e-11
    finally:
        ctx.set_grid_limit(0)

    # -- a slice gives bit for bit the rows of the whole
    if n >= 3:
        at = 0
        for part in ds.chunks(3):
            _, _, up, dp, lp, _ = model._estep(part, u=True, maha=True, llks=True)
            sl = slice(at, at + len(part))
            assert np.array_equal(up, u[sl]) and np.array_equal(dp, delta[sl]) and np.array_equal(lp, ell[sl])
            at += len(part)
        assert at == n


@functools.lru_cache(maxsize=None)
def _sweep_want(d, k, nu):
    x, w, (s, c, mu) = S.robust_case(d, k)
    return R.estep(x, w, s, c, mu, nu)


@pytest.mark.parametrize("d", S.ROBUST_DS)
@pytest.mark.parametrize("k", S.KS)
def test_state_size_sweep(P, k, d):
    """Every instantiation of the sweep: the four row blocks KB = 4, 8, 12, 16 (with every k that pads a thread's rows of C) x the three
    column layouts (d <= 64, d <= 256, beyond) x the three modes that the E-step check's calls reach, at n = 70 (a ragged last step in
    every layout); then one ECM step (d = 300: the EM pass on the scaled rows runs through the lane solver).  Rows 0 .. k + 2 hold
    exactly 0 .. k + 2 entries."""
    nu = 4.0
    case, e = S.robust_case(d, k), _sweep_want(d, k, nu)
    assert np.array_equal(e["m"][:k + 3], np.arange(k + 3))
    _check_estep(P, case, e, nu)
    x, w, (s, c, mu) = case
    model = P.TPPCAModel(s, c, mu, nu)
    new, llk = model.iterate_with_llk(P.Dataset(x, w))
    errs = _model_errors(new, R.mstep(s, c, mu, e))
    errs["llk"] = abs(llk - e["scalars"][1]) / e["scalars_abs"][1]
    print("   iterate 70x%dx%d" % (d, k), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("nu", [0.7, 200.0])
def test_estep_other_degrees_of_freedom(P, nu):
    n, d, k = 600, 256, 10
    x, w, (s, c, mu) = _case(n, d, k)
    got = P.TPPCAModel(s, c, mu, nu)._estep(P.Dataset(x, w), scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True)
    errs = _estep_errors(got, _want(n, d, k, nu), d, k)
    print("estep nu=%g" % nu, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs


def test_estep_on_an_empty_dataset(P):
    model = P.TPPCAModel(1.0, np.ones((5, 2)), np.zeros(5), 4.0)
    y, cs, u, delta, ell, sc = model._estep(P.Dataset(np.empty((0, 5))), scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True)
    assert len(y) == 0 and np.array_equal(cs, np.zeros(25)) and u.shape == (0,) and np.array_equal(sc, np.zeros(4))


def _model_errors(new, want):
    s1, c1, m1 = want
    return dict(sigma=abs(new.isotropic_noise / s1 - 1), C=float(np.abs(new.transform - c1).max() / np.abs(c1).max()),
                mean=float((np.abs(new.mean - m1) / np.maximum(np.abs(m1), s1)).max()))


STEP_SHAPES = [(3000, 256, 10), (2000, 200, 16), (1500, 300, 4), (400, 1024, 16)]


@pytest.mark.parametrize("n,d,k", STEP_SHAPES, ids=["%dx%dx%d" % s for s in STEP_SHAPES])
def test_iterate_against_restatement(P, n, d, k):
    nu = 4.0
    x, w, (s, c, mu) = _case(n, d, k)
    e = _want(n, d, k, nu)
    ds = P.Dataset(x, w)
    model = P.TPPCAModel(s, c, mu, nu)
    new, llk = model.iterate_with_llk(ds)
    errs = _model_errors(new, R.mstep(s, c, mu, e))
    errs["llk"] = abs(llk - e["scalars"][1]) / e["scalars_abs"][1]
    errs["llk_vs_llk()"] = abs(llk - model.llk(ds)) / abs(llk)
    print("iterate %dx%dx%d" % (n, d, k), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g; llk() 1e-12)" % TOL)
    assert max(errs["sigma"], errs["C"], errs["mean"], errs["llk"]) <= TOL and errs["llk_vs_llk()"] <= 1e-12, errs
    assert new.dof == nu and new.n_parameters == model.n_parameters
    plain = model.iterate(ds)
    assert plain.isotropic_noise == new.isotropic_noise and np.array_equal(plain.transform, new.transform) and np.array_equal(plain.mean, new.mean)
    est = model.iterate(ds, estimate_dof=True)
    want_nu = R.dof_root(e["scalars"][2] / e["scalars"][0])
    print("   nu %.9g, restatement %.9g" % (est.dof, want_nu))
    assert abs(est.dof / want_nu - 1) <= 1e-6 and np.array_equal(est.transform, new.transform)
    assert est.n_parameters == model.n_parameters + 1


N_MASK = 293
MASK_SHAPES = [(256, 10), (200, 16), (300, 4)]


@pytest.mark.parametrize("name", MP.NAMES)
@pytest.mark.parametrize("d,k", MASK_SHAPES, ids=["d%d-k%d" % s for s in MASK_SHAPES])
def test_structured_masks(P, oracle, d, k, name):
    nu = 4.0
    x, w, (s, c, mu), mask = MP.case(oracle, N_MASK, d, k, name, 3000 + 7 * d + k)
    e = R.estep(x, w, s, c, mu, nu)
    ds = P.Dataset(x, w)
    model = P.TPPCAModel(s, c, mu, nu)
    errs = _estep_errors(model._estep(ds, scaled=True, col_sums=True, u=True, maha=True, llks=True, scalars=True), e, d, k)
    new, llk = model.iterate_with_llk(ds)
    errs.update(_model_errors(new, R.mstep(s, c, mu, e)))
    errs["llk"] = abs(llk - e["scalars"][1]) / max(e["scalars_abs"][1], 1.0)
    print("masks d%d k%d %s" % (d, k, name), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs
    never = ~mask.any(0)
    assert np.array_equal(new.transform[never], c[never]) and np.array_equal(new.mean[never], mu[never])


@pytest.mark.parametrize("estimate", [False, True], ids=["nu-fixed", "nu-estimated"])
def test_llk_never_decreases(P, estimate):
    rng = np.random.default_rng(21)
    n, d, k = 20000, 64, 5
    x = rng.standard_normal((n, k)) @ rng.standard_normal((d, k)).T + 0.5 * rng.standard_normal((n, d)) / np.sqrt(rng.gamma(2.0, 0.5, n))[:, None]
    x[rng.random(x.shape) < 0.3] = np.nan
    ds = P.Dataset(x, rng.uniform(0.5, 2.0, n))
    model, prev = P.TPPCAModel.init(k, ds, seed=3, dof=4.0), -np.inf
    for it in range(25):
        model, llk = model.iterate_with_llk(ds, estimate_dof=estimate)
        assert llk >= prev - 1e-9 * abs(llk), (it, llk, prev)
        prev = llk
    print("llk %.6f sigma %.4f nu %.3f" % (prev, model.isotropic_noise, model.dof))


def test_gaussian_limit_of_llks(P):
    n, d, k = 500, 32, 4
    x, w, (s, c, mu) = _case(n, d, k)
    ds = P.Dataset(x, w)
    t, g = P.TPPCAModel(s, c, mu, 1e9).llks(ds), P.PPCAModel(s, c, mu).llks(ds)
    err = _rel(t, g)
    print("nu = 1e9: llks against PPCAModel.llks %.1e (bound 1e-6: the t density is O(m^2 / nu) from the Gaussian)" % err)
    assert err <= 1e-6


def test_contaminated_case(P):
    x, c_true, bad, c0 = R.contaminated_start()
    ds = P.Dataset(x)
    d = x.shape[1]
    t = P.TPPCATrainer(ds).train(state_size=3, dof=4.0, n_iters=30, start=P.TPPCAModel(1.0, c0, np.zeros(d), 4.0), quiet=True)
    g = P.PPCATrainer(ds).train(state_size=3, n_iters=30, start=P.PPCAModel(1.0, c0, np.zeros(d)), quiet=True)
    at, ag = R.subspace_angle(t.transform, c_true), R.subspace_angle(g.transform, c_true)
    u = t.row_weights(ds)
    print("t: %.2f degrees, sigma %.3f; Gaussian: %.2f degrees, sigma %.3f; median u contaminated %.3f clean %.3f"
          % (at, t.isotropic_noise, ag, g.isotropic_noise, np.median(u[bad]), np.median(u[~bad])))
    assert at < 5.0 and ag > 20.0
    assert np.median(u[bad]) < 0.1 and np.median(u[~bad]) > 0.5


def test_unsupported_shapes_launch_nothing(P):
    from ppca_rs_amd import _lib

    L = _lib.lib()
    with pytest.raises(ValueError):
        P.TPPCAModel.init(0, P.Dataset(np.zeros((4, 3))))
    with pytest.raises(ValueError):
        P.TPPCAModel(1.0, np.zeros((3, 0)), np.zeros(3), 4.0)
    for d, k in ((20, 17), (1025, 2)):
        ds = P.Dataset(np.random.default_rng(0).standard_normal((8, d)))
        ctx = ds._ctx
        g = P.PPCAModel(1.0, np.ones((d, k)), np.zeros(d))
        dev = g._device(ctx)
        ctx.enable_timing(True)
        try:
            ctx.kernel_time(reset=True)
            out = np.empty(8)
            rc = L.ppca_t_estep(ctx.handle, ds._h, dev.h, 4.0, None, None, _lib.ptr(out), None, None, None)
            assert rc == -3 and "covers state sizes 1 .. 16 and output sizes 1 .. 1024" in L.ppca_last_error().decode()
            s1, c1, m1 = C.c_double(0.0), np.empty((d, k)), np.empty(d)
            rc = L.ppca_t_em_step(ctx.handle, ds._h, d, k, 1.0, _lib.ptr(np.ones((d, k))), _lib.ptr(np.zeros(d)), 4.0, C.byref(s1),
                                  _lib.ptr(c1), _lib.ptr(m1), None, None)
            assert rc == -3 and "covers state sizes" in L.ppca_last_error().decode()
            with pytest.raises(_lib.PPCAError):
                _lib.check(rc)
            assert ctx.kernel_time(reset=True)[1] == 0  # nothing was launched
        finally:
            ctx.enable_timing(False)
        with pytest.raises(ValueError, match="covers state sizes"):
            P.TPPCAModel(1.0, np.ones((d, k)), np.zeros(d), 4.0)
