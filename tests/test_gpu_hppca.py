"""PPCA with a known precision per entry on the GPU (HPPCAModel): the E-step sweep, the statistics contraction,
the reconstructions and the ECM step against the row-by-row restatement (tests/hppca_restatement.py) and against the library's own
PPCAModel and FAModel where the models coincide; what the sweep promises exactly (per-row outputs that do not depend on the grid, a
slice or the chunk); structured masks; errors; and the property that justifies the model.

Tolerance: the project's GPU parity tolerance, 1e-5, with the measures of tests/test_gpu_robust.py: per row relative to 1 + |value|,
sums relative to the sum of their terms' magnitudes; sigma relative, C against max |C|, mean_j against max(|mean_j|, sigma).  Each
parity check prints its worst error before asserting."""
import functools
import os
import pickle

import numpy as np
import pytest

import hppca_restatement as R
import mask_patterns as MP
import state_size_cases as S

pytestmark = pytest.mark.gpu

TOL = 1e-5
INVALID = -1


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(n, d, k, lo=2.0 ** -10, hi=2.0 ** 10):
    x, p, w, model = R.case(n, d, k, 2000 + 31 * n + 7 * d + k, lo, hi)
    _freeze(x, p, w, *model[1:])
    return x, p, w, model


@functools.lru_cache(maxsize=None)
def _want(n, d, k, lo=2.0 ** -10, hi=2.0 ** 10):
    x, p, w, (s, c, mu) = _case(n, d, k, lo, hi)
    return R.estep(x, p, w, s, c, mu)


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _sum_err(got, want, scale):
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())


def _estep_errors(got, e):
    ll, st, cv, ss, sc = got
    return dict(ell=_rel(ll, e["ell"]), z=_rel(st, e["z"]), Sigma=_rel(cv, e["Sigma"]),
                stats=_sum_err(ss, R.packed_stats(e), R.packed_stats(e, "abs")), scalars=_sum_err(sc[:3], e["scalars"], e["scalars_abs"]))


def _model_errors(new, want):
    s1, c1, m1 = want
    return dict(sigma=abs(new.isotropic_noise / s1 - 1), C=float(np.abs(new.transform - c1).max() / np.abs(c1).max()),
                mean=float((np.abs(new.mean - m1) / np.maximum(np.abs(m1), s1)).max()))


def _all(model, ds, prec):
    return model._estep(ds, prec, llks=True, states=True, covs=True, stats=True, scalars=True)


# the issue's shapes, then the edges of the tiling as built: a column just past a 32-column table chunk (33), three 16-column blocks
# of vech(c c^T) and a record of exactly nine blocks (k = 15), a second [w z | w] block (k = 16, above), 96 = 3 chunks with k = 11
SHAPES = [(1, 1, 1), (3, 5, 2), (65, 17, 3), (257, 64, 10), (130, 65, 16), (600, 256, 10), (300, 257, 4), (2000, 200, 16), (200, 1024, 16),
          (70, 33, 5), (100, 96, 11), (40, 31, 15)]


@pytest.mark.parametrize("n,d,k", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_against_restatement(P, n, d, k):
    _check_against_restatement(P, _case(n, d, k), _want(n, d, k))


@functools.lru_cache(maxsize=None)
def _sweep_want(k):
    x, p, w, (s, c, mu) = S.hetero_case(k)
    return R.estep(x, p, w, s, c, mu)


@pytest.mark.parametrize("k", S.KS)
def test_state_size_sweep(P, k):
    """Every instantiation of the sweep and the statistics kernel at (130, 97, k): two full 64-row workgroup steps and one of 2 rows,
    eight 16-row steps of the statistics kernel and 2 rows; three column chunks of 32 and one column (k = 11, 12: one of 64 and 33
    columns), one full 64-column tile of the statistics kernel and a ragged one.  Rows 0 .. k + 2 hold exactly 0 .. k + 2 entries."""
    e = _sweep_want(k)
    assert np.array_equal(e["m"][:k + 3], np.arange(k + 3))
    _check_against_restatement(P, S.hetero_case(k), e)


def _check_against_restatement(P, case, e):
    x, p, w, (s, c, mu) = case
    (n, d), k = x.shape, c.shape[1]
    ds, prec = P.Dataset(x, w), P.Dataset(p)
    model = P.HPPCAModel(s, c, mu)
    got = _all(model, ds, prec)
    errs = _estep_errors(got, e)
    print("estep %dx%dx%d" % (n, d, k), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs
    ll, st, cv, ss, sc = got
    empty = e["m"] == 0
    assert np.all(ll[empty] == 0) and not st[empty].any() and sc[2] == (~empty).sum() and sc[3] == 0

    # -- the narrower calls return the same numbers; an array of precisions is a Dataset of them
    assert np.array_equal(model.llks(ds, prec), ll) and np.array_equal(model.llks(ds, p), ll)
    inf = model.infer(ds, prec)
    assert np.array_equal(inf.states(), st) and np.array_equal(np.array(inf.covariances()), cv)
    assert model.llk(ds, prec) == sc[1]

    # -- smooth / extrapolate
    zs = e["z"]
    sm, ex = model.smooth(ds, prec), model.extrapolate(ds, prec)
    rerr = dict(smooth=_rel(sm.numpy(), R.reconstruct(x, p, c, mu, zs, 0)), extrapolate=_rel(ex.numpy(), R.reconstruct(x, p, c, mu, zs, 1)))
    print("   recon", " ".join("%s %.1e" % kv for kv in rerr.items()))
    assert max(rerr.values()) <= TOL, rerr
    obs = R.observed(x, p)
    assert np.array_equal(ex.numpy()[obs], x[obs]) and np.array_equal(ex.weights(), w)

    # -- one iteration
    new, llk = model.iterate_with_llk(ds, prec)
    merr = _model_errors(new, R.mstep(s, c, mu, e))
    print("   iterate", " ".join("%s %.1e" % kv for kv in merr.items()))
    assert max(merr.values()) <= TOL, merr
    assert llk == model.llk(ds, prec)  # bit for bit
    again = model.iterate(ds, prec)
    assert again.isotropic_noise == new.isotropic_noise and np.array_equal(again.transform, new.transform)

    # -- under a capped grid: per-row outputs bit for bit, the sums to 1e-11
    ctx = ds._ctx
    mag = R.packed_stats(e, "abs")
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            lg, sg, cg, ssg, scg = _all(model, ds, prec)
            assert np.array_equal(lg, ll) and np.array_equal(sg, st) and np.array_equal(cg, cv)
            assert _sum_err(ssg, ss, mag) <= 1e-11 and _sum_err(scg[:3], sc[:3], e["scalars_abs"]) <= 1e-11
    finally:
        ctx.set_grid_limit(0)

    # -- a slice of dataset and precisions gives bit for bit the rows of the whole
    if n >= 3:
        at = 0
        for part, ppart in zip(ds.chunks(3), prec.chunks(3)):
            lp, sp, cp, _, _ = model._estep(part, ppart, llks=True, states=True, covs=True)
            sl = slice(at, at + len(part))
            assert np.array_equal(lp, ll[sl]) and np.array_equal(sp, st[sl]) and np.array_equal(cp, cv[sl])
            at += len(part)
        assert at == n

    # -- a forced small chunk gives the same per-row bits
    if n >= 65:
        os.environ["PPCA_H_CHUNK"] = "48"
        try:
            lc, sc_, cc, ssc, scc = _all(model, ds, prec)
            smc = model.smooth(ds, prec).numpy()
        finally:
            del os.environ["PPCA_H_CHUNK"]
        assert np.array_equal(lc, ll) and np.array_equal(sc_, st) and np.array_equal(cc, cv) and np.array_equal(smc, sm.numpy())
        assert _sum_err(ssc, ss, mag) <= 1e-11 and _sum_err(scc[:3], sc[:3], e["scalars_abs"]) <= 1e-11


def test_unit_precisions_equal_ppcamodel(P):
    n, d, k = 600, 256, 10
    x, _, w, (s, c, mu) = _case(n, d, k)
    ds, ones = P.Dataset(x, w), np.ones_like(x)
    h, g = P.HPPCAModel(s, c, mu), P.PPCAModel(s, c, mu)
    hi, gi = h.infer(ds, ones), g.infer(ds)
    errs = dict(llks=_rel(h.llks(ds, ones), g.llks(ds)), states=_rel(hi.states(), gi.states()),
                covs=_rel(np.array(hi.covariances()), np.array(gi.covariances())),
                smooth=_rel(h.smooth(ds, ones).numpy(), g.smooth(ds).numpy()),
                extrapolate=_rel(h.extrapolate(ds, ones).numpy(), g.extrapolate(ds).numpy()))
    print("p = 1 against PPCAModel", " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs


def test_column_precisions_equal_famodel(P):
    n, d, k = 300, 257, 4
    x, _, w, (_, c, mu) = _case(n, d, k)
    psi = np.random.default_rng(3).uniform(0.2, 2.0, d)
    ds, prec = P.Dataset(x, w), np.broadcast_to(1.0 / psi ** 2, x.shape).copy()
    h, f = P.HPPCAModel(1.0, c, mu), P.FAModel(psi, c, mu)
    errs = dict(llks=_rel(h.llks(ds, prec), f.llks(ds)), states=_rel(h.infer(ds, prec).states(), f.infer(ds).states()))
    print("p = 1 / psi^2 against FAModel", " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs


PATTERN_SHAPE = (200, 130, 4)


@functools.lru_cache(maxsize=None)
def _pattern_case(name, on_precisions):
    n, d, k = PATTERN_SHAPE
    x, p, w, model = R.case(n, d, k, 77)
    mask = MP.patterns(n, d, k, 77)[name]
    if on_precisions:  # x full; the pattern is the zero pattern of the precisions
        rng = np.random.default_rng(78)
        x = np.where(np.isfinite(x), x, rng.standard_normal((n, d)))
        p = np.where(mask, np.where(R.observed(np.zeros_like(p), p), p, 1.0), 0.0)
    else:
        x = np.where(mask, np.where(np.isfinite(x), x, 0.25), np.nan)
    _freeze(x, p, w)
    s, c, mu = model
    return x, p, w, model, R.estep(x, p, w, s, c, mu)


@pytest.mark.parametrize("on_precisions", [False, True], ids=["x-mask", "p-zeros"])
@pytest.mark.parametrize("name", MP.NAMES)
def test_structured_masks(P, name, on_precisions):
    x, p, w, (s, c, mu), e = _pattern_case(name, on_precisions)
    ds, prec = P.Dataset(x, w), P.Dataset(p)
    model = P.HPPCAModel(s, c, mu)
    errs = _estep_errors(_all(model, ds, prec), e)
    new = model.iterate(ds, prec)
    errs.update(_model_errors(new, R.mstep(s, c, mu, e)))
    print("pattern %s" % name, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs
    for j in np.flatnonzero(e["T"] == 0):  # an all-empty column keeps its mean and its row of C
        assert new.mean[j] == mu[j] and np.array_equal(new.transform[j], c[j])
    if name in ("rank_edge", "column_once"):
        assert (e["m"] == 0).any() or (e["T"] == 0).any()


# Precisions over twelve orders of magnitude.  On this case the restatement's two forms differ by at most 3.7e-10 (per row) and 2.9e-10
# of sum |terms| (statistics), below TOL / 10, so the range [1e-6, 1e6] is used as it is.
WIDE = (300, 40, 6, 1e-6, 1e6)


def test_wide_range_of_precisions(P):
    n, d, k, lo, hi = WIDE
    x, p, w, (s, c, mu) = _case(n, d, k, lo, hi)
    a, b = R.estep(x, p, w, s, c, mu, dense=True), R.estep(x, p, w, s, c, mu, dense=False)
    forms = max(max(_rel(a[key], b[key]) for key in ("ell", "z", "Sigma")),
                _sum_err(R.packed_stats(b), R.packed_stats(a), R.packed_stats(a, "abs")))
    print("restatement's two forms on [%g, %g]: %.1e" % (lo, hi, forms))
    assert forms <= TOL / 10
    model, ds, prec = P.HPPCAModel(s, c, mu), P.Dataset(x, w), P.Dataset(p)
    errs = _estep_errors(_all(model, ds, prec), a)
    errs.update(_model_errors(model.iterate(ds, prec), R.mstep(s, c, mu, a)))
    print("wide range", " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("bad", [-1.0, np.inf, -np.inf], ids=["negative", "+inf", "-inf"])
def test_bad_precisions_are_an_error(P, bad):
    n, d, k = 130, 65, 16
    x, p, w, (s, c, mu) = _case(n, d, k)
    p = p.copy()
    p[97, 40] = bad
    ds, prec, model = P.Dataset(x, w), P.Dataset(p), P.HPPCAModel(s, c, mu)
    out = np.full(n, 123.0)
    with pytest.raises(P.PPCAError, match="negative or \\+inf") as err:
        P.api.check(P.api.lib().ppca_h_estep(ds._ctx.handle, ds._h, prec._h, model._base._device(ds._ctx).h, P.api.ptr(out), None, None,
                                             None, None))
    assert err.value.code == INVALID and np.all(out == 123.0)  # no output
    for call in (model.llks, model.infer, model.smooth, model.extrapolate, model.iterate, model.iterate_with_llk, model.llk):
        with pytest.raises(P.PPCAError) as err:
            call(ds, prec)
        assert err.value.code == INVALID


def test_shape_mismatch_is_an_error(P):
    x, p, w, (s, c, mu) = _case(65, 17, 3)
    ds, model = P.Dataset(x, w), P.HPPCAModel(s, c, mu)
    for other in (p[:64], p[:, :16]):
        with pytest.raises(ValueError):
            model.llks(ds, other)
    for other in (P.Dataset(p[:64].copy()), P.Dataset(p[:, :16].copy())):
        with pytest.raises(P.PPCAError) as err:
            model.llks(ds, other)
        assert err.value.code == INVALID
    with pytest.raises(ValueError):
        model.iterate(P.Dataset(np.empty((0, 17))), np.empty((0, 17)))


def test_empty_dataset(P):
    model = P.HPPCAModel(1.0, np.ones((5, 2)), np.zeros(5))
    ll, st, cv, ss, sc = _all(model, P.Dataset(np.empty((0, 5))), np.empty((0, 5)))
    assert ll.shape == (0,) and not ss.any() and np.array_equal(sc, np.zeros(4))


def test_true_precisions_find_the_subspace(P):
    """The property that justifies the model: entries at two noise levels, 0.3 and 3.0.  The restatement on the CPU ends 4.48 degrees
    from the true subspace with the true precisions and 19.59 degrees with every precision 1 (R.HETERO_ANGLES); the GPU fit with
    the true precisions must beat the Gaussian fit by half that gap."""
    x, p, c_true, c0 = R.hetero_case()
    margin = 0.5 * (R.HETERO_ANGLES[1] - R.HETERO_ANGLES[0])
    ds, prec = P.Dataset(x), P.Dataset(p)
    h, g = P.HPPCAModel(1.0, c0, np.zeros(x.shape[1])), P.PPCAModel(1.0, c0, np.zeros(x.shape[1]))
    for _ in range(R.HETERO["iters"]):
        h, g = h.iterate(ds, prec), g.iterate(ds)
    ah, ag = R.subspace_angle(h.transform, c_true), R.subspace_angle(g.transform, c_true)
    print("true precisions: %.3f degrees; PPCAModel: %.3f degrees (margin %.3f)" % (ah, ag, margin))
    assert ah + margin < ag


def test_trainer_and_persistence(P):
    n, d, k = 600, 12, 3
    x, p, w, _ = _case(n, d, k)
    ds = P.Dataset(x, w)
    model, metrics = P.HPPCATrainer(ds, p).train(state_size=k, n_iters=10, seed=5)
    llk = [m.llk for m in metrics]
    print("trainer llk per row:", " ".join("%.4f" % v for v in llk))
    assert len(metrics) == 10 and all(isinstance(m, P.TrainMetrics) for m in metrics)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(llk, llk[1:]))
    assert isinstance(model, P.HPPCAModel) and np.allclose(model.transform, model.to_canonical().transform, rtol=0, atol=1e-9)  # canonical
    start = P.HPPCAModel.init(k, ds, seed=5)
    assert metrics[0].llk == start.llk(ds, p) / n
    assert P.HPPCAModel.init(k, ds, method="pca").state_size == k
    for back in (P.HPPCAModel.load(model.dump()), pickle.loads(pickle.dumps(model))):
        assert np.array_equal(back.llks(ds, p), model.llks(ds, p))
    drawn = model.sample(p, seed=1)
    assert np.array_equal(np.isnan(drawn.numpy()), ~R.observed(np.zeros_like(p), p))
