"""Every path on data in other units: the exact power-of-two rescaling of tests/units_cases.py on the GPU.

Every other test of the suite feeds the library numbers of order one.  Here the data, the mean and the loadings are multiplied by
a = 2^p (p = +40 and -40: 1e+12 and 1e-12) and the noise level by a, and the run is compared with the SAME build's run on the unscaled
inputs (pinned to the oracle by the rest of the suite): posteriors, unit-free statistics, z-scores, labels and draws bit for bit,
everything with units as an exact power of two, log-likelihoods by the derived 16-ulp relation.  The sample weights times 2^q
(q = +30, -30) likewise.  Engines, guards and fallbacks must not move.  Every tolerance in this file is zero, the 16-ulp llk bound
(units_cases.llk_bound; with units_cases.log_sum_bound where a family adds a sum of library logarithms) or the measured mixture bound.
"""
import ctypes as C

import numpy as np
import pytest

import units_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@pytest.fixture()
def ctx(P):
    from ppca_rs_amd import _lib

    c = _lib.default_context()
    c.set_grid_limit(0)
    c.set_heavy_rows(8)
    yield c
    c.set_grid_limit(0)
    c.set_heavy_rows(8)


def _engine(ds, m):
    from ppca_rs_amd import _lib

    e = C.c_int32(-1)
    _lib.check(_lib.lib().ppca_gram_engine(ds._ctx.handle, m._device(ds._ctx).h, C.byref(e)))
    return e.value


def _stats(ds, m):
    from ppca_rs_amd import _lib

    got = np.empty(_lib.lib().ppca_stats_len(m.output_size, max(m.state_size, 1)))
    _lib.check(_lib.lib().ppca_stats_raw(ds._ctx.handle, ds._h, m._device(ds._ctx).h, _lib.ptr(got)))
    return got


def _verdict(ctx, ds, m):
    """What the EM pass that has just run decided, in a form that must not move with the units -- of THAT pass: the fused eight-wave
    kernel (k <= 10) files its guards' verdicts and its fallback (ppca_em_last_guard / ppca_em_last_fallback report the most recent
    FUSED pass only); the two-kernel pass and the split pipeline leave the dispatch record of ppca_generic_last_trace, checked to be
    this pass's.  Both with the diagnostic counters of the int8 statistics contraction since the reset in front of the pass (exponents
    raised, flushes, tiles walked, launches)."""
    from ppca_rs_amd import _lib

    d, k, n = m.output_size, max(m.state_size, 1), len(ds)
    counters = tuple(ctx.debug_counters(reset=True))
    if k <= 10 and _lib.lib().ppca_path_kind(d, k) == 1:
        return ("fused", ctx.last_guard(), ctx.last_fallback()[:3], counters)
    t = ctx.generic_trace()
    assert t["valid"] == 1 and t["em"] == 1 and (t["d"], t["k"], t["n"]) == (d, k, n), ("not this pass's record", t)
    return ("record", t, counters)


def _cov_diag(P, ds, m, mode):
    from ppca_rs_amd import _lib

    h = C.c_void_p()
    _lib.check(_lib.lib().ppca_covariance_diagonal(ds._ctx.handle, ds._h, m._device(ds._ctx).h, mode, C.byref(h)))
    return P.Dataset._wrap(h, ds._ctx).numpy()


def _model_of(m):
    return dict(sigma=m.isotropic_noise, transform=m.transform, mean=m.mean)


def _score_of(hs):
    cols = hs.columns
    return dict(count=cols["count"], col_llk=cols["llk"], se=cols["se"], z2=cols["z2"], llks=hs.llks, llk=hs.llk, mse=hs.mse,
                mean_z2=hs.mean_z2, n_entries=hs.n_entries, n_rows=hs.n_rows, total_count=hs.count)


def _assert_model(got, base, p, what):
    for key in ("sigma", "transform", "mean"):
        U.assert_pow2(got[key], base[key], p, what + (key,))


def _assert_score(got, base, p, what, held_obs, w, extra_rows=0.0, extra_cols=0.0, extra_total=0.0):
    """A HeldOutScore of the scaled run: counts and z2 identical, se and mse times a^2, the three llks by the relation."""
    for key in ("count", "z2", "mean_z2", "n_entries", "n_rows", "total_count"):
        U.assert_bits(got[key], base[key], what + (key,))
    U.assert_pow2(got["se"], base["se"], 2 * p, what + ("se",))
    U.assert_pow2(got["mse"], base["mse"], 2 * p, what + ("mse",))
    assert base["n_entries"] > 0
    U.assert_llk(got["llks"], base["llks"], held_obs.sum(axis=1), p, what + ("held llks",), extra_rows)
    U.assert_llk(got["col_llk"], base["col_llk"], base["count"], p, what + ("held llk by column",), extra_cols)
    U.assert_llk(got["llk"], base["llk"], base["total_count"], p, what + ("held llk",), extra_total)


# --------------------------------------------------------------------------- PPCAModel
def _run_ppca(P, ctx, cs, p, variant, q=0):
    """Every output of PPCAModel on the case in units 2^p (weights times 2^q): a dict of host arrays and scalars."""
    x = U.scaled_data(cs["x"], p)
    s, c, mu = U.scaled_model(cs["sigma"], cs["c"], cs["mu"], p)
    w = U.pow2(cs["w"], q) if variant == "weighted" else None
    ctx.set_grid_limit(1 if variant == "grid1" else 0)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    out = dict(engine=_engine(ds, m))
    ctx.debug_counters(reset=True)
    out["stats"] = _stats(ds, m)
    out["verdict"] = _verdict(ctx, ds, m)
    inf = m.infer(ds)
    out["states"], out["covs"] = inf.states(), np.array(inf.covariances())
    out["smooth"], out["extrapolate"] = m.smooth(ds).numpy(), m.extrapolate(ds).numpy()
    out["sm_diag"] = inf.smoothed_covariances_diagonal(m).numpy()
    out["ex_diag"] = inf.extrapolated_covariances_diagonal(m, ds).numpy()
    out["dev_sm_diag"], out["dev_ex_diag"] = _cov_diag(P, ds, m, 0), _cov_diag(P, ds, m, 1)
    it = m.iterate(ds)
    out["iterate_verdict"] = _verdict(ctx, ds, m)
    out["iterate"] = _model_of(it)
    it_llk, out["em_llk"] = m.iterate_with_llk(ds)
    out["iterate_with_llk"] = _model_of(it_llk)
    third = it.iterate(ds).iterate(ds)  # (the finaliser of each step builds the digit table of the next)
    out["third"] = _model_of(third)
    out["llks"], out["llk"] = m.llks(ds), m.llk(ds)
    loo = m.loo_predictive(ds)
    out["loo_mean"], out["loo_var"], out["loo_z"] = loo.mean().numpy(), loo.variance().numpy(), loo.zscores()
    out["loo_llks"], out["loo_llk"] = loo.llks(), loo.llk()
    out["draw"] = m.sample_posterior(ds, seed=7).numpy()
    out["imputed"] = m.sample_posterior(ds, seed=7, keep_observed=True).numpy()
    train, held = ds.holdout(0.2, 11)
    out["train"], out["held"], out["split_counts"] = train.numpy(), held.numpy(), train.holdout_counts
    out["score"] = _score_of(m.heldout_score(train, held))
    ctx.set_grid_limit(0)
    return out


def _compare_ppca(got, base, cs, p, variant, what):
    d, k = cs["c"].shape
    obs = np.isfinite(cs["x"])
    m_i = obs.sum(axis=1)
    w = cs["w"] if variant == "weighted" else np.ones(len(m_i))
    assert m_i[cs["empty"]] == 0 and (m_i > 0).sum() == len(m_i) - 1
    assert got["engine"] == base["engine"], (what, "engine", got["engine"], base["engine"])
    assert got["verdict"] == base["verdict"], (what, "verdict", got["verdict"], base["verdict"])
    assert got["iterate_verdict"] == base["iterate_verdict"], (what, "verdict of iterate")
    for key in ("states", "covs"):
        U.assert_bits(got[key], base[key], what + (key,))
    for key in ("smooth", "extrapolate", "loo_mean", "draw", "imputed"):
        U.assert_pow2(got[key], base[key], p, what + (key,))
    for key in ("sm_diag", "ex_diag", "dev_sm_diag", "dev_ex_diag", "loo_var"):
        U.assert_pow2(got[key], base[key], 2 * p, what + (key,))
    U.assert_bits(got["loo_z"], base["loo_z"], what + ("loo z-scores",), where=obs)
    for key in ("iterate", "iterate_with_llk", "third"):
        _assert_model(got[key], base[key], p, what + (key,))
    wm = float(np.dot(w, m_i))
    U.assert_stats(got["stats"], base["stats"], d, max(k, 1), p, 0, what + ("stats",), llk_cnt=wm)
    U.assert_llk(got["llks"], base["llks"], m_i, p, what + ("llks",))
    U.assert_llk(got["llk"], base["llk"], wm, p, what + ("llk",))
    U.assert_llk(got["em_llk"], base["em_llk"], wm, p, what + ("llk of the EM pass",))
    U.assert_llk(got["loo_llks"], base["loo_llks"], m_i, p, what + ("loo_llks",))
    U.assert_llk(got["loo_llk"], base["loo_llk"], wm, p, what + ("loo_llk",))
    assert got["split_counts"] == base["split_counts"] and base["split_counts"][1] > 0
    for key in ("train", "held"):
        part = np.isfinite(base[key])
        assert np.array_equal(np.isfinite(got[key]), part), what + (key, "other cells")
        U.assert_pow2(got[key], base[key], p, what + (key,), where=part)
    _assert_score(got["score"], base["score"], p, what, np.isfinite(base["held"]), w)


_BASE = {}


def _base_ppca(P, ctx, shape, variant, mean_scale=1.0):
    key = (shape, variant, mean_scale)
    if key not in _BASE:
        cs = U.make_case(*shape, mean_scale=mean_scale)
        _BASE[key] = (cs, _run_ppca(P, ctx, cs, 0, variant))
    return _BASE[key]


IDS = ["%dx%dx%d" % s for s in U.SHAPES]


@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("variant", U.VARIANTS)
@pytest.mark.parametrize("shape", U.SHAPES, ids=IDS)
def test_ppca_model_in_other_units(P, ctx, shape, variant, p):
    """Every pass of PPCAModel on the fused eight-wave kernel, the two-kernel pass, the split pipeline (lane, batched and blocked
    solvers) and state size 0, with 30 % of the entries masked and a row with nothing observed: un-weighted on the full grid, weighted,
    and on one workgroup that walks every tile."""
    cs, base = _base_ppca(P, ctx, shape, variant)
    _compare_ppca(_run_ppca(P, ctx, cs, p, variant), base, cs, p, variant, (shape, variant, p))


@pytest.mark.parametrize("shape", [(200, 256, 10), (130, 200, 16), (60, 300, 4)], ids=["fused", "two-kernel", "split"])
def test_ppca_model_far_from_zero(P, ctx, shape):
    """The asymmetric case: data times 2^40 whose mean lies 50 standard deviations of the means' spread from zero, so that x - mean
    cancels many leading bits of entries at 1e14."""
    cs, base = _base_ppca(P, ctx, shape, "weighted", mean_scale=50.0)
    _compare_ppca(_run_ppca(P, ctx, cs, 40, "weighted"), base, cs, 40, "weighted", (shape, "mean_scale 50"))


EDGES = [((200, 256, 10), 90), ((200, 256, 10), -90), ((130, 200, 16), 56), ((130, 200, 16), -56), ((64, 70, 20), 200), ((64, 70, 20), -200)]


@pytest.mark.parametrize("shape,p", EDGES, ids=["%dx%dx%d-p%+d" % (s + (p,)) for s, p in EDGES])
def test_ppca_model_at_the_edges_of_the_documented_range(P, ctx, shape, p):
    """The range DESIGN.md section 7 guarantees, per engine.  The fused passes take det M as two products of ceil(k / 2) pivots, each
    pivot between sigma^2 and sigma^2 + |C|^2 in the data's units: five pivots (k <= 10) stay inside a double for order-one data times
    2^+-90 (1e+-27), eight (k <= 16) for 2^+-56 (1e+-17); the split pipeline splits every pivot and is bounded by the fourth powers
    of the noise level instead: 2^+-200 (1e+-60)."""
    cs, base = _base_ppca(P, ctx, shape, "plain")
    _compare_ppca(_run_ppca(P, ctx, cs, p, "plain"), base, cs, p, "plain", (shape, "edge", p))


@pytest.mark.parametrize("q", U.WEIGHT_POWERS, ids=["q+30", "q-30"])
@pytest.mark.parametrize("shape", [(200, 256, 10), (130, 200, 16), (60, 300, 4)], ids=["fused", "two-kernel", "split"])
def test_weights_in_other_units(P, ctx, shape, q):
    """with_weights(w 2^q) rescales [wP | wz | w]: every exponent E_c of the fixed-point form, the first-scale rule and the heavy-row
    test move.  Every entry of the statistics is 2^q times the unscaled one (the count of non-empty samples stays), the llk is exactly
    2^q times, the new model is bit-identical and the verdicts do not move."""
    cs, base = _base_ppca(P, ctx, shape, "weighted")
    d, k = cs["c"].shape
    ds = P.Dataset(cs["x"], cs["w"]).with_weights(U.pow2(cs["w"], q))
    m = P.PPCAModel(cs["sigma"], cs["c"], cs["mu"])
    what = (shape, "weights", q)
    ctx.debug_counters(reset=True)
    got = _stats(ds, m)
    assert _verdict(ctx, ds, m) == base["verdict"], what
    U.assert_stats(got, base["stats"], d, k, 0, q, what + ("stats",))
    new, llk = m.iterate_with_llk(ds)
    assert _verdict(ctx, ds, m) == base["iterate_verdict"], what
    _assert_model(_model_of(new), base["iterate"], 0, what + ("iterate",))
    U.assert_pow2(llk, base["em_llk"], q, what + ("llk of the EM pass",))
    U.assert_pow2(m.llk(ds), base["llk"], q, what + ("llk",))
    U.assert_bits(m.llks(ds), base["llks"], what + ("llks",))
    assert _engine(ds, m) == base["engine"]


# --------------------------------------------------------------------------- engines and guards
def _guard_models(rng):
    """Three models built like those of tests/test_gpu_parity.py::test_int8_gram_dynamic_range_guard (the same constructions on data drawn
    here, not that test's arrays; the p = 0 asserts confirm the engines they reach): (name, x, w, sigma, c, mu, engine)."""
    d, k, n = 256, 10, 640
    big = np.sort(rng.choice(d, 200, replace=False))
    mu = 0.1 * rng.standard_normal(d)
    out = []
    c0 = rng.standard_normal((d, k))
    x0 = rng.standard_normal((n, k)) @ rng.standard_normal((k, d)) + 0.1 * rng.standard_normal((n, d))
    x0[rng.random((n, d)) < 0.3] = np.nan
    out.append(("benign", x0, None, 0.1, c0, mu, 0))
    cd = rng.standard_normal((d, k))
    cd[5] *= 1.0e-2
    xd = rng.standard_normal((n, k)) @ cd.T + mu + 1.0e-3 * rng.standard_normal((n, d))
    xd[rng.random((n, d)) < 0.3] = np.nan
    out.append(("trained", xd, None, 1.0e-3, cd, mu, 0))
    scale = np.ones(d)
    scale[big] = 1.0e8
    c = rng.standard_normal((d, k)) * scale[:, None]
    x = rng.standard_normal((n, k)) @ c.T + mu + 0.05 * rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    x[:, big] = np.nan
    out.append(("rows spanning 1e8", x, rng.uniform(0.5, 1.5, n), 0.05, c, mu, 1))
    return out


def test_gram_guard_verdicts_in_other_units(P, ctx):
    """A benign model of the headline shape, a "trained" model (sigma = 1e-3, one weak row) and a guard-tripping model (rows of C
    spanning 1e8, the large ones masked everywhere), built like those of test_int8_gram_dynamic_range_guard, go to engines 0, 0, 1 at
    p = 0, +40 and -40, and the statistics of each follow the exact relation.

    The llk scalar of the "trained" model, and of that model alone, needs more than the 16-ulp bound, for a stated reason (measured
    at p = +40: 117 times that bound, 1.6e-6 of an llk of 2.6e6); the other two are held to the 16-ulp bound.  em9_kernel adds a row's small terms, 2 ln sigma (m - k) + ln(2 pi) m
    and the log-determinant, to -quad_i / sigma^2 and subtracts sum |x~|^2 / sigma^2 once per workgroup (sample_llk_nolog with xx = 0):
    with sigma = 1e-3 a row's quad / sigma^2 is 2e9 against an llk of 9e2, so the terms that move with the units are rounded at
    ulp(2e9), at p = 0 as well -- a loss of the pass's llk to cancellation at small noise levels (1e-10 relative here, inside what
    the suite asks of it against the oracle), not a dependence on the units.  Bounded by its rounding count instead: with
    Q = sum_i w_i |x~_i|^2 / sigma^2 >= sum_i w_i quad_i / sigma^2, per run two roundings of the row's sum at Q_i, one each of the
    determinant's addition and the weight's product at Q_i / 2, the T running additions of a lane (T tiles per workgroup, 1 on the
    full grid at n = 640) and the five levels of the wave's sum at (sum Q) / 2: (5.5 + T / 2) 2^-53 Q, twice for the two runs."""
    for name, x, w, s, c, mu, engine in _guard_models(np.random.default_rng(77)):
        d, k = c.shape
        ww = np.ones(len(x)) if w is None else w
        wm = float(np.dot(ww, np.isfinite(x).sum(axis=1)))
        big_q = float(np.dot(ww, np.where(np.isfinite(x), (x - mu) ** 2, 0.0).sum(axis=1))) / (s * s)
        base = None
        for p in (0,) + U.POWERS:
            ds, m = P.Dataset(U.scaled_data(x, p), w), P.PPCAModel(*U.scaled_model(s, c, mu, p))
            assert _engine(ds, m) == engine, (name, p)
            got = dict(stats=_stats(ds, m), verdict=(ctx.last_guard(), ctx.last_fallback()[:3]), states=m.infer(ds).states())
            if p == 0:
                base = got
                assert got["verdict"][0][0] == engine
                continue
            assert got["verdict"] == base["verdict"], (name, p)
            extra = 6.0 * 2.0 ** -52 * big_q if name == "trained" else 0.0
            U.assert_stats(got["stats"], base["stats"], d, k, p, 0, (name, p), llk_cnt=wm, llk_extra=extra)
            U.assert_bits(got["states"], base["states"], (name, p, "states"))


@pytest.mark.parametrize("heavy_max", [8, 0])
def test_outlier_row_verdicts_in_other_units(P, ctx, heavy_max):
    """A dataset like that of test_outlier_rows_go_round_the_fixed_point_form (one row times 1e6, here on 600 rows of
    units_cases.make_case; the p = 0 assert confirms the verdicts it is about): with heavy_max = 8 the row goes round the
    fixed-point form and no guard trips; with 0 the W-side guard sends its workgroup to the fp64 stage.  The same verdicts and
    bit-identical statistics after un-scaling at p = +40 and -40, on the full grid and on one workgroup."""
    n, d, k = 600, 256, 10
    cs = U.make_case(n, d, k, seed=6)
    x = cs["x"].copy()
    x[100] *= 1e6
    wm = float(np.isfinite(x).sum())
    for cap in (0, 1):
        base = None
        for p in (0,) + U.POWERS:
            ctx.set_heavy_rows(heavy_max)
            ctx.set_grid_limit(cap)
            ds, m = P.Dataset(U.scaled_data(x, p)), P.PPCAModel(*U.scaled_model(cs["sigma"], cs["c"], cs["mu"], p))
            got = dict(stats=_stats(ds, m), verdict=(ctx.last_guard(), ctx.last_fallback()[:3]))
            if p == 0:
                base = got
                assert (got["verdict"][0] == (0, 0)) == (heavy_max == 8), (heavy_max, cap, got["verdict"])
                continue
            assert got["verdict"] == base["verdict"], (heavy_max, cap, p, got["verdict"], base["verdict"])
            U.assert_stats(got["stats"], base["stats"], d, k, p, 0, ("outlier", heavy_max, cap, p), llk_cnt=wm)


# --------------------------------------------------------------------------- SparseDataset
@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("shape", [(64, 9, 3), (150, 300, 11), (100, 20, 0)], ids=["64x9x3", "150x300x11", "100x20x0"])
def test_sparse_dataset_in_other_units(P, ctx, shape, p):
    """iterate, llks, llk, infer, predict and heldout_score on row-compressed data (70 % of the entries missing)."""
    cs = U.make_case(*shape, mask=0.7)
    obs = np.isfinite(cs["x"])
    m_i = obs.sum(axis=1)
    wm = float(np.dot(cs["w"], m_i))

    def run(pp):
        sp = P.SparseDataset.from_dense(U.scaled_data(cs["x"], pp), cs["w"])
        m = P.PPCAModel(*U.scaled_model(cs["sigma"], cs["c"], cs["mu"], pp))
        inf = m.infer(sp)
        new, llk = m.iterate_with_llk(sp)
        train, held = sp.holdout(0.2, 11)
        return dict(states=inf.states(), covs=np.array(inf.covariances()), iterate=_model_of(new), em_llk=llk, llks=m.llks(sp), llk=m.llk(sp),
                    predict=m.predict(sp, sp), held=held._dense(), score=_score_of(m.heldout_score(train, held)))

    base, got = run(0), run(p)
    what = (shape, "sparse", p)
    U.assert_bits(got["states"], base["states"], what + ("states",))
    U.assert_bits(got["covs"], base["covs"], what + ("covs",))
    _assert_model(got["iterate"], base["iterate"], p, what)
    U.assert_pow2(got["predict"][0], base["predict"][0], p, what + ("predictive mean",))
    U.assert_pow2(got["predict"][1], base["predict"][1], 2 * p, what + ("predictive variance",))
    U.assert_llk(got["llks"], base["llks"], m_i, p, what + ("llks",))
    U.assert_llk(got["llk"], base["llk"], wm, p, what + ("llk",))
    U.assert_llk(got["em_llk"], base["em_llk"], wm, p, what + ("llk of the EM pass",))
    assert np.array_equal(np.isfinite(got["held"]), np.isfinite(base["held"]))
    _assert_score(got["score"], base["score"], p, what, np.isfinite(base["held"]), cs["w"])


# --------------------------------------------------------------------------- FAModel
@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("shape", [(150, 40, 3), (100, 64, 20)], ids=["fused", "split"])
def test_fa_model_in_other_units(P, ctx, shape, p):
    """Per-column noise times a: the whitened rows are bit-identical, so are the posteriors; smooth, extrapolate and the new model
    scale exactly.  The log-likelihoods add sum_j ln noise_j over the observed entries, numpy's logarithm of a scaled argument summed
    on the device: units_cases.log_sum_bound on top of the llk bound."""
    cs = U.make_case(*shape)
    n, d = cs["x"].shape
    psi = np.random.default_rng(8).uniform(0.4, 1.6, d)
    obs = np.isfinite(cs["x"])
    m_i = obs.sum(axis=1)
    w = cs["w"]

    def run(pp):
        ds = P.Dataset(U.scaled_data(cs["x"], pp), w)
        m = P.FAModel(*U.scaled_fa(psi, cs["c"], cs["mu"], np.array(pp)))
        inf = m.infer(ds)
        new, llk = m.iterate_with_llk(ds)
        train, held = ds.holdout(0.2, 11)
        return dict(states=inf.states(), covs=np.array(inf.covariances()), smooth=m.smooth(ds).numpy(), extrapolate=m.extrapolate(ds).numpy(),
                    new=dict(noise=new.noise, transform=new.transform, mean=new.mean), em_llk=llk, llks=m.llks(ds), llk=m.llk(ds),
                    held=held.numpy(), score=_score_of(m.heldout_score(train, held)))

    base, got = run(0), run(p)
    what = (shape, "FA", p)
    U.assert_bits(got["states"], base["states"], what + ("states",))
    U.assert_bits(got["covs"], base["covs"], what + ("covs",))
    for key in ("smooth", "extrapolate"):
        U.assert_pow2(got[key], base[key], p, what + (key,))
    for key in ("noise", "transform", "mean"):
        U.assert_pow2(got["new"][key], base["new"][key], p, what + (key,))
    ln = np.abs(np.log(psi)) + abs(p) * U.LN2  # |ln(noise_j 2^p)| <= this
    rows = U.log_sum_bound(m_i, obs @ ln)
    total = U.log_sum_bound(d, (w @ obs) @ ln)  # (llk and the step's llk subtract ONE dot product of the column totals with ln noise)
    U.assert_llk(got["llks"], base["llks"], m_i, p, what + ("llks",), rows)
    U.assert_llk(got["llk"], base["llk"], float(np.dot(w, m_i)), p, what + ("llk",), total)
    U.assert_llk(got["em_llk"], base["em_llk"], float(np.dot(w, m_i)), p, what + ("llk of the EM pass",), total)
    hobs = np.isfinite(base["held"])
    assert np.array_equal(np.isfinite(got["held"]), hobs)
    hrows = U.log_sum_bound(hobs.sum(axis=1), hobs @ ln)
    hcols = U.log_sum_bound(1, (w @ hobs) * ln)
    _assert_score(got["score"], base["score"], p, what, hobs, w, hrows, hcols, float(hcols.sum()))


# --------------------------------------------------------------------------- TPPCAModel
@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("shape", [(65, 17, 3), (100, 300, 4), (130, 200, 16)], ids=["65x17x3", "100x300x4", "130x200x16"])
def test_t_model_in_other_units(P, ctx, shape, p):
    """The Student-t family: dof does not move; row weights and Mahalanobis distances are unit-free, bit for bit; estimate_dof gives
    the same dof bit for bit (q, the sum it is the root of, is unit-free)."""
    cs = U.make_case(*shape)
    obs = np.isfinite(cs["x"])
    m_i = obs.sum(axis=1)
    w = cs["w"]
    wm = float(np.dot(w, m_i))

    def run(pp):
        ds = P.Dataset(U.scaled_data(cs["x"], pp), w)
        m = P.TPPCAModel(*U.scaled_model(cs["sigma"], cs["c"], cs["mu"], pp), 4.0)
        new, llk = m.iterate_with_llk(ds)
        est = m.iterate(ds, estimate_dof=True)
        delta, cnt = m.mahalanobis(ds)
        train, held = ds.holdout(0.2, 11)
        return dict(u=m.row_weights(ds), delta=delta, cnt=cnt, states=m.infer(ds).states(), smooth=m.smooth(ds).numpy(),
                    new=_model_of(new), new_dof=new.dof, est=_model_of(est), est_dof=est.dof, em_llk=llk, llks=m.llks(ds), llk=m.llk(ds),
                    held=held.numpy(), score=_score_of(m.score_heldout(train, held)))

    base, got = run(0), run(p)
    what = (shape, "t", p)
    for key in ("u", "delta", "cnt", "states", "new_dof", "est_dof"):
        U.assert_bits(got[key], base[key], what + (key,))
    assert base["est_dof"] != 4.0 and base["new_dof"] == 4.0
    U.assert_pow2(got["smooth"], base["smooth"], p, what + ("smooth",))
    _assert_model(got["new"], base["new"], p, what + ("iterate",))
    _assert_model(got["est"], base["est"], p, what + ("iterate, dof estimated",))
    U.assert_llk(got["llks"], base["llks"], m_i, p, what + ("llks",))
    U.assert_llk(got["llk"], base["llk"], wm, p, what + ("llk",))
    U.assert_llk(got["em_llk"], base["em_llk"], wm, p, what + ("llk of the ECM pass",))
    _assert_score(got["score"], base["score"], p, what, np.isfinite(base["held"]), w)


# --------------------------------------------------------------------------- HPPCAModel
@pytest.mark.parametrize("mode", ["p+40", "p-40", "columns"])
@pytest.mark.parametrize("shape", [(65, 17, 3), (100, 96, 11)], ids=["65x17x3", "100x96x11"])
def test_known_precision_model_in_other_units(P, ctx, shape, mode):
    """The noise variance of an entry is sigma^2 / p_ij: data times a_j with the noise level as it is and the precisions times a_j^-2
    (one power for every column, +40 and -40; and one power p_j in [-20, 20] per column) -- loadings and mean times a_j, the new noise
    level, the posteriors and the statistics' unit-free blocks bit for bit.  The log-density carries sum_O ln p_ij, one device logarithm
    per entry of a scaled argument: the llk bound with cnt = sum_O p_j."""
    cs = U.make_case(*shape)
    n, d = cs["x"].shape
    rng = np.random.default_rng(12)
    prec = np.exp2(rng.uniform(-3.0, 3.0, (n, d)))
    pj = np.full(d, 40) if mode == "p+40" else np.full(d, -40) if mode == "p-40" else rng.integers(-20, 21, d)
    obs = np.isfinite(cs["x"])
    w = cs["w"]

    def run(pv):
        ds = P.Dataset(U.scaled_data(cs["x"], pv), w)
        pr = U.scaled_precisions(prec, pv)
        m = P.HPPCAModel(cs["sigma"], *U.scaled_columns(cs["c"], cs["mu"], pv))
        inf = m.infer(ds, pr)
        new, llk = m.iterate_with_llk(ds, pr)
        train, held = ds.holdout(0.2, 11)
        return dict(states=inf.states(), covs=np.array(inf.covariances()), smooth=m.smooth(ds, pr).numpy(), new=_model_of(new), em_llk=llk,
                    llks=m.llks(ds, pr), llk=m.llk(ds, pr), held=held.numpy(), score=_score_of(m.score_heldout(train, held, pr)))

    base, got = run(np.zeros(d, dtype=np.int64)), run(pj)
    what = (shape, "known precisions", mode)
    U.assert_bits(got["states"], base["states"], what + ("states",))
    U.assert_bits(got["covs"], base["covs"], what + ("covs",))
    U.assert_pow2(got["smooth"], base["smooth"], pj, what + ("smooth",))
    U.assert_bits(got["new"]["sigma"], base["new"]["sigma"], what + ("sigma",))
    U.assert_pow2(got["new"]["transform"], base["new"]["transform"], pj[:, None], what + ("transform",))
    U.assert_pow2(got["new"]["mean"], base["new"]["mean"], pj, what + ("mean",))
    # the relation with "cnt p" = sum_O p_j (assert_llk takes (cnt, p) = (that sum, 1)) and, in the bound, sum_O |p_j|: where the
    # powers have both signs the shifts cancel and the roundings do not, so the difference of the two enters as `extra`
    shift, mag = obs @ pj, obs @ np.abs(pj)
    for key, cnt, cmag in (("llks", shift, mag), ("llk", float(w @ shift), float(w @ mag)), ("em_llk", float(w @ shift), float(w @ mag))):
        extra = U.LLK_ULPS * 2.0 ** -52 * (np.asarray(cmag, dtype=np.float64) - np.abs(cnt)) * U.LN2
        U.assert_llk(got[key], base[key], cnt, 1, what + (key,), extra)
    hobs = np.isfinite(base["held"])
    assert np.array_equal(np.isfinite(got["held"]), hobs)
    gs, bs = got["score"], base["score"]
    for key in ("count", "z2", "mean_z2", "n_entries", "n_rows", "total_count"):
        U.assert_bits(gs[key], bs[key], what + (key,))
    U.assert_pow2(gs["se"], bs["se"], 2 * pj, what + ("se",))
    hshift, hmag = hobs @ pj, hobs @ np.abs(pj)
    U.assert_llk(gs["llks"], bs["llks"], hshift, 1, what + ("held llks",), U.LLK_ULPS * 2.0 ** -52 * (hmag - np.abs(hshift)) * U.LN2)
    U.assert_llk(gs["col_llk"], bs["col_llk"], bs["count"] * pj, 1, what + ("held llk by column",))
    tshift, tmag = float(bs["count"] @ pj), float(bs["count"] @ np.abs(pj))
    U.assert_llk(gs["llk"], bs["llk"], tshift, 1, what + ("held llk",), U.LLK_ULPS * 2.0 ** -52 * (tmag - abs(tshift)) * U.LN2)
    if mode != "columns":  # (one power for every column: the mean squared error is an exact multiple too)
        U.assert_pow2(gs["mse"], bs["mse"], 2 * int(pj[0]), what + ("mse",))


# --------------------------------------------------------------------------- k-means, pairwise moments, column statistics
@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("shape,nc", [((257, 64), 3), ((120, 514), 9)], ids=["257x64-K3", "120x514-K9"])
def test_kmeans_in_other_units(P, ctx, shape, nc, p):
    """One Lloyd step (one read of the dataset; and d > 512 with K > 8: assignment and update sweeps per block of centres) and a whole
    seeded run: labels, totals, counts, iterations identical; centres and sums times a; distances and inertia times a^2."""
    n, d = shape
    cs = U.make_case(n, d, 2)
    centers = cs["mu"] + np.random.default_rng(4).standard_normal((nc, d))

    def run(pp):
        ds = P.Dataset(U.scaled_data(cs["x"], pp), cs["w"])
        st = ds.kmeans_step(U.pow2(centers, pp), distances=True)
        km = ds.kmeans(nc, n_iters=5, seed=3)
        return st, km

    (bst, bkm), (gst, gkm) = run(0), run(p)
    what = (shape, nc, p)
    assert gst.reads == bst.reads
    U.assert_bits(gst.labels, bst.labels, what + ("labels",))
    U.assert_bits(gst.totals, bst.totals, what + ("totals",))
    U.assert_pow2(gst.sums, bst.sums, p, what + ("sums",))
    U.assert_pow2(gst.centers(), bst.centers(), p, what + ("new centres",))
    U.assert_pow2(gst.distances, bst.distances, 2 * p, what + ("distances",))
    U.assert_pow2(gst.inertia, bst.inertia, 2 * p, what + ("inertia",))
    assert (gkm.n_iters_run, gkm.converged) == (bkm.n_iters_run, bkm.converged)
    U.assert_bits(gkm.labels, bkm.labels, what + ("kmeans labels",))
    U.assert_bits(gkm.cluster_weights, bkm.cluster_weights, what + ("cluster weights",))
    U.assert_pow2(gkm.centers, bkm.centers, p, what + ("kmeans centres",))
    U.assert_pow2(gkm.history, bkm.history, 2 * p, what + ("history",))
    U.assert_pow2(gkm.inertia, bkm.inertia, 2 * p, what + ("kmeans inertia",))


@pytest.mark.parametrize("p", U.POWERS, ids=["p+40", "p-40"])
@pytest.mark.parametrize("shape", [(65, 17), (257, 130)], ids=["65x17", "257x130"])
def test_moments_and_column_stats_in_other_units(P, ctx, shape, p):
    """pairwise_moments (one tile pair, and several): sums times a^2, cross and centre times a, counts identical, the correlation bit
    for bit in both modes; column_stats: totals identical, means times a, variances times a^2."""
    n, d = shape
    cs = U.make_case(n, d, 2)

    def run(pp):
        ds = P.Dataset(U.scaled_data(cs["x"], pp), cs["w"])
        return ds.pairwise_moments(cross=True), ds.column_stats()

    (bm, bc), (gm, gc) = run(0), run(p)
    what = (shape, p)
    U.assert_bits(gm.counts, bm.counts, what + ("counts",))
    U.assert_pow2(gm.center, bm.center, p, what + ("centre",))
    U.assert_pow2(gm.sums, bm.sums, 2 * p, what + ("sums",))
    U.assert_pow2(gm.cross, bm.cross, p, what + ("cross",))
    for mode in ("global", "pairwise"):
        ok = np.isfinite(bm.correlation(mode))
        assert ok.sum() > d
        U.assert_bits(gm.correlation(mode), bm.correlation(mode), what + ("correlation", mode), where=ok)
        U.assert_pow2(gm.covariance(mode), bm.covariance(mode), 2 * p, what + ("covariance", mode), where=np.isfinite(bm.covariance(mode)))
    U.assert_bits(gc[0], bc[0], what + ("totals",))
    U.assert_pow2(gc[1], bc[1], p, what + ("means",))
    U.assert_pow2(gc[2], bc[2], 2 * p, what + ("variances",))


# --------------------------------------------------------------------------- the mixtures
MIX_SHAPES = [(300, 24, 3, 3), (200, 40, 6, 2)]  # n, d, k, components: k <= 6, where the oracle's determinant stays finite at 2^+-20
MIX_POWERS = (20, -20)


def _mix_case(n, d, k, nm):
    """Components that OVERLAP (close means, loadings around a shared one), so that the responsibilities of many rows are graded: with
    well-separated clusters they saturate at 0 and 1 and the step is bit-exact for the wrong reason."""
    rng = np.random.default_rng(900 + d)
    parts, models = [], []
    shared = rng.standard_normal((d, k))
    for q in range(nm):
        c, mu = shared + 0.3 * rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d)
        xq = rng.standard_normal((n // nm, k)) @ c.T + mu + 0.5 * rng.standard_normal((n // nm, d))
        parts.append(xq)
        models.append((0.5, c + 0.2 * rng.standard_normal((d, k)), mu + 0.1 * rng.standard_normal(d)))
    x = np.concatenate(parts)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[len(x) // 3] = np.nan
    return x, rng.uniform(0.25, 2.0, len(x)), models, np.log(rng.dirichlet(5.0 * np.ones(nm)))


def _mixture(scale, transforms, means, log_weights, per_column=False):
    """A mixture as four arrays: scale (the components' noise levels, or FAMix's per-column noise), transforms (components, d, k), means
    (components, d), log-weights; per_column: the scale is one noise level per column, not one per component."""
    return dict(per_column=per_column, scale=np.asarray(scale, dtype=np.float64), transforms=np.stack([np.asarray(c) for c in transforms]),
                means=np.stack([np.asarray(m) for m in means]), log_weights=np.asarray(log_weights, dtype=np.float64))


def _mix_discrepancy(got, base, p, what):
    """The worst relative discrepancy, after un-scaling, of a new mixture (_mixture) against the unscaled run's: the scale entry by
    entry, every C_c of its largest entry, the means of max(|mean|, the scale that belongs to the entry: the component's noise level, or
    the column's) and the log-weights absolutely.  Every array of both runs is asserted finite first: a NaN must not pass as 0."""
    for key in ("scale", "transforms", "means", "log_weights"):
        U.assert_finite(got[key], what + (key, "scaled run"))
        U.assert_finite(base[key], what + (key, "unscaled run"))
        assert got[key].shape == base[key].shape, what + (key,)
    s0 = base["scale"]
    ref = s0[None, :] if base["per_column"] else s0[:, None]
    figs = [np.abs(got["log_weights"] - base["log_weights"]).max(), np.abs(U.unscale(got["scale"], p) / s0 - 1.0).max(),
            (np.abs(U.unscale(got["transforms"], p) - base["transforms"]).max(axis=(1, 2)) / np.abs(base["transforms"]).max(axis=(1, 2))).max(),
            (np.abs(U.unscale(got["means"], p) - base["means"]) / np.maximum(np.abs(base["means"]), ref)).max()]
    worst = float(np.max(figs))
    assert np.isfinite(worst), what
    return worst


_MIX_BOUND = []


def _oracle_mix_bound(oracle):
    """EIGHT times the worst relative discrepancy, after un-scaling, of the fp64 oracle's mix_iterate between the scaled and the unscaled
    run, over every case of MIX_SHAPES and both MIX_POWERS (k <= 6 and 2^+-20: the oracle's literal determinant is checked finite
    first).  Computed once."""
    if not _MIX_BOUND:
        worst = 0.0
        for n, d, k, nm in MIX_SHAPES:
            x, w, models, lw = _mix_case(n, d, k, nm)
            sig, cc, mm = np.array([m[0] for m in models]), np.stack([m[1] for m in models]), np.stack([m[2] for m in models])

            def run(pp):
                xs = U.scaled_data(x, pp)
                args = (xs, np.ldexp(sig, pp), U.pow2(cc, pp), U.pow2(mm, pp), lw)
                assert np.isfinite(oracle.mix_llks(*args)).all(), "the oracle's determinant left the range"
                return _mixture(*oracle.mix_iterate(*args, w))

            base = run(0)
            for p in MIX_POWERS:
                fig = _mix_discrepancy(run(p), base, p, ("oracle", (n, d, k, nm), p))
                print("oracle mix_iterate %dx%dx%d-m%d p=%+d: %.3e" % (n, d, k, nm, p, fig))
                worst = max(worst, fig)
        _MIX_BOUND.append(8.0 * worst)
    return _MIX_BOUND[0]


@pytest.mark.parametrize("n,d,k,nm", MIX_SHAPES, ids=["300x24x3-m3", "200x40x6-m2"])
def test_ppca_mixture_in_other_units(P, oracle, ctx, n, d, k, nm):
    """PPCAMix.  The responsibilities pass through exp of log-likelihood differences, so iterate is not bit-exact; llks follow the llk
    relation at p = +40, -40 (every component's llk shifts by the same m_i p ln 2) and infer_cluster gives the same labels on every row
    whose two largest log-posteriors differ by more than 1e-6.  iterate at p = +20, -20 is held to EIGHT times the worst relative
    discrepancy of the fp64 oracle's own mix_iterate between its scaled and unscaled runs of the same cases (_oracle_mix_bound: the
    device sums in another order over the same conditioning).
    Measured: the oracle's worst figure is 1.89e-15 (300x24x3-m3 at p = +20; 1.78e-15 at -20; 200x40x6-m2: 4.6e-16 .. 7.8e-16 with
    its thread count), so the bound is 1.51e-14; the device's discrepancy is 5.79e-15 / 4.15e-15 (300x24x3-m3, p = +20 / -20) and
    2.94e-15 / 2.82e-15 (200x40x6-m2)."""
    x, w, models, lw = _mix_case(n, d, k, nm)
    m_i = np.isfinite(x).sum(axis=1)

    def mix(pp):
        return P.PPCAMix([P.PPCAModel(*U.scaled_model(s, c, mu, pp)) for s, c, mu in models], lw)

    ds0 = P.Dataset(x, w)
    base_llks, base_lp = mix(0).llks(ds0), mix(0).infer_cluster(ds0)
    U.assert_finite(base_lp, "log posteriors")
    top = np.sort(base_lp, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-6
    assert clear.sum() > n // 2
    assert (np.exp(top[:, -1]) < 0.99).sum() >= 5  # (rows whose responsibilities are graded: the exp is really exercised)
    for p in U.POWERS:
        dsp = P.Dataset(U.scaled_data(x, p), w)
        U.assert_llk(mix(p).llks(dsp), base_llks, m_i, p, ("mixture llks", p))
        lp = mix(p).infer_cluster(dsp)
        U.assert_finite(lp, ("log posteriors", p))
        assert np.array_equal(lp.argmax(axis=1)[clear], base_lp.argmax(axis=1)[clear]), ("labels", p)

    def dev_iter(pp):
        new = mix(pp).iterate(P.Dataset(U.scaled_data(x, pp), w))
        return _mixture([m.isotropic_noise for m in new.models], [m.transform for m in new.models], [m.mean for m in new.models], new.log_weights)

    bound = _oracle_mix_bound(oracle)
    dev0 = dev_iter(0)
    for p in MIX_POWERS:
        dev = _mix_discrepancy(dev_iter(p), dev0, p, ("device", (n, d, k, nm), p))
        print("mixture iterate %dx%dx%d-m%d p=%+d: device %.3e bound %.3e" % (n, d, k, nm, p, dev, bound))
        assert dev <= bound, (p, dev, bound)


@pytest.mark.parametrize("n,d,k,nm", MIX_SHAPES[:1], ids=["300x24x3-m3"])
def test_fa_mixture_in_other_units(P, ctx, n, d, k, nm):
    """FAMix: llks by the relation (with the Jacobian sum of FAModel), the same labels on the clear rows, and iterate at p = +20, -20
    held to eight times the discrepancy of tests/famix_restatement.py (dense numpy, fp64) between its scaled and unscaled runs.
    Measured: the restatement 4.44e-15 / 3.55e-15 (p = +20 / -20), the device 0 / 0 -- the whitened rows are unit-free, so the whole
    step is bit-identical after un-scaling and only the products with the noise levels at its end see the units."""
    import famix_restatement as R

    x, w, models, lw = _mix_case(n, d, k, nm)
    psi = np.random.default_rng(8).uniform(0.4, 1.6, d)
    obs = np.isfinite(x)
    m_i = obs.sum(axis=1)
    cc, mm = np.stack([m[1] for m in models]), np.stack([m[2] for m in models])

    def mix(pp):
        return P.FAMix(U.pow2(psi, pp), U.pow2(cc, pp), U.pow2(mm, pp), lw)

    ds0 = P.Dataset(x, w)
    base_llks, base_lp = mix(0).llks(ds0), mix(0).infer_cluster(ds0)
    U.assert_finite(base_lp, "log posteriors")
    top = np.sort(base_lp, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-6
    assert clear.sum() > n // 2
    for p in U.POWERS:
        dsp = P.Dataset(U.scaled_data(x, p), w)
        ln = np.abs(np.log(psi)) + abs(p) * U.LN2
        U.assert_llk(mix(p).llks(dsp), base_llks, m_i, p, ("FA mixture llks", p), U.log_sum_bound(m_i, obs @ ln))
        lp = mix(p).infer_cluster(dsp)
        U.assert_finite(lp, ("log posteriors", p))
        assert np.array_equal(lp.argmax(axis=1)[clear], base_lp.argmax(axis=1)[clear]), ("labels", p)

    def dev_iter(pp):
        new = mix(pp).iterate(P.Dataset(U.scaled_data(x, pp), w))
        return _mixture(new.noise, new.transforms, new.means, new.log_weights, per_column=True)

    def ref_iter(pp):
        out = R.iterate(U.scaled_data(x, pp), w, U.pow2(psi, pp), list(U.pow2(cc, pp)), list(U.pow2(mm, pp)), lw)
        return _mixture(out[0], out[1], out[2], out[3], per_column=True)

    ref0, dev0 = ref_iter(0), dev_iter(0)
    for p in MIX_POWERS:
        ref = _mix_discrepancy(ref_iter(p), ref0, p, ("restatement", p))
        dev = _mix_discrepancy(dev_iter(p), dev0, p, ("device", p))
        print("FA mixture iterate %dx%dx%d-m%d p=%+d: restatement %.3e device %.3e bound %.3e" % (n, d, k, nm, p, ref, dev, 8.0 * ref))
        assert dev <= 8.0 * ref, (p, dev, ref)
