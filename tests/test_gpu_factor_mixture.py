"""The mixture of factor analysers with shared column noise on the GPU: the multi-component column sweep against numpy, FAMix's llks /
infer_cluster / iterate / smooth against the dense restatement in original units (tests/famix_restatement.py), and the properties of
the model -- a step that equals FAModel's at one component, commutes with rescaling columns and never lowers the log-likelihood.

Tolerance: the project's GPU parity tolerance, 1e-5 relative (psi per element; C against max |C|; mean_cj against max(|mean_cj|, psi_j);
a row's llk against |llk| + d; log-weights absolute), unless a check names its own bound.  Each parity check prints its worst error
before asserting."""
import numpy as np
import pytest

import famix_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _mix_errors(got, want):
    """(psi, C, mean, log-weights) worst errors of an FAMix against the restatement's (psi, [C_c], [mean_c], log-weights)."""
    p0, c0, m0, l0 = want
    ec = max(np.abs(got.transforms[q] - c0[q]).max() / np.abs(c0[q]).max() for q in range(len(c0)))
    em = max((np.abs(got.means[q] - m0[q]) / np.maximum(np.abs(m0[q]), p0)).max() for q in range(len(c0)))
    return np.abs(got.noise / p0 - 1).max(), ec, em, np.abs(got.log_weights - l0).max()


# --------------------------------------------------------------------------- the sweep against numpy
N_PASS = 3001


def _sweep_inputs(d, nc, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_PASS + 40, d)) * rng.uniform(0.1, 10.0, d) + rng.standard_normal(d)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[9 + 23] = np.nan  # an all-masked row (inside both the plain rows and the slice)
    x[11 + 23, d // 2] = np.inf  # masked like every non-finite entry
    x[:, d - 1] = np.where(np.arange(x.shape[0]) % 97 == 0, x[:, d - 1], np.nan)  # a nearly empty column
    e = rng.uniform(0.0, 1.0, (nc, x.shape[0])) ** 4  # (most of a row's weight in few components, as responsibilities)
    e[:, 40] = 0.0  # a row no component weighs
    e[nc - 1, 50] = np.nan  # a non-finite weight counts as 0
    a = rng.uniform(0.2, 5.0, d) * rng.choice([-1.0, 1.0], d)
    # offsets 1e3 column standard deviations apart from the first component to the last
    mean, std = np.nanmean(np.where(np.isfinite(x), x, np.nan), 0) * a, np.nanstd(np.where(np.isfinite(x), x, np.nan), 0) * np.abs(a)
    b = mean + np.linspace(0.0, 1e3, nc)[:, None] * std * rng.choice([-1.0, 1.0], d)
    return x, e, a, b


def _sweep_reference(x, e, a, b):
    obs = np.isfinite(x)
    y = np.where(obs, x, 0.0) * a
    sums, scale = np.empty((e.shape[0], 3, x.shape[1])), np.empty((e.shape[0], 3, x.shape[1]))
    for c in range(e.shape[0]):
        wm = np.where(np.isfinite(e[c]), e[c], 0.0)[:, None] * obs
        r = np.where(obs, y - b[c], 0.0)
        sums[c] = wm.sum(0), (wm * r).sum(0), (wm * r * r).sum(0)
        scale[c] = sums[c, 0], (wm * np.abs(r)).sum(0), sums[c, 2]  # what each sum is a sum OF: the measure of its rounding
    return sums, scale


@pytest.mark.parametrize("sliced", [False, True], ids=["plain", "slice"])
@pytest.mark.parametrize("nc", [1, 2, 3, 4, 5, 8, 9, 16])  # (KB = 1, 2, 4, 8: a partial and a full block of each, two full trips)
@pytest.mark.parametrize("d", [256, 200, 1024, 7])
def test_multi_component_sweep_against_numpy(P, d, nc, sliced):
    """Every sum within 1e-12 of numpy's, relative to the sum of the absolute values of its terms (the bound and measure of
    test_scale_pass_against_numpy).  With the offsets 1e3 standard deviations apart, a kernel that squared around a common pivot and
    corrected afterwards would lose six digits of sq to the cancellation."""
    x, e, a, b = _sweep_inputs(d, nc, 300 + 16 * d + nc)
    lo = 23 if sliced else 0  # (an odd first row: with d = 7 the slice's rows are not 16-byte aligned)
    ds = P.Dataset(x)._slice(lo, N_PASS) if sliced else P.Dataset(np.ascontiguousarray(x[:N_PASS]))
    xs, es = x[lo:lo + N_PASS], np.ascontiguousarray(e[:, lo:lo + N_PASS])
    sums, scale = _sweep_reference(xs, es, a, b)
    got = ds._column_moments_multi(es, a, b)
    err = np.abs(got - sums) / np.where(scale > 0, scale, 1.0)
    print(f"d={d} K={nc}: worst column sum {err.max():.2e} (bound 1e-12)")
    assert got.shape == (nc, 3, d) and err.max() <= 1e-12
    assert np.all(got[scale == 0] == 0.0)
    assert np.array_equal(ds._column_moments_multi(es, a, b), got)  # two runs are bit-identical
    ctx = ds._ctx
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            assert (np.abs(ds._column_moments_multi(es, a, b) - sums) / np.where(scale > 0, scale, 1.0)).max() <= 1e-12
    finally:
        ctx.set_grid_limit(0)


@pytest.mark.parametrize("d", [256, 7])
def test_multi_component_sweep_special_inputs(P, d):
    """One component weighted by the dataset's own weights, no offset: the sums of the scale pass.  a and b are nullable."""
    rng = np.random.default_rng(d)
    x = rng.standard_normal((N_PASS, d)) * rng.uniform(0.1, 10.0, d)
    x[rng.random(x.shape) < 0.3] = np.nan
    w, a = rng.uniform(0.5, 2.0, N_PASS), rng.uniform(0.2, 5.0, d)
    ds = P.Dataset(x, w)
    want = ds._scale_columns(a, out=False, col_sums=True)[1]
    got = ds._column_moments_multi(w[None, :], a)
    obs = np.isfinite(x)
    wm = w[:, None] * obs
    scale = np.stack([wm.sum(0), (wm * np.abs(np.where(obs, x * a, 0.0))).sum(0), (wm * np.where(obs, x * a, 0.0) ** 2).sum(0)])
    err = np.abs(got[0] - want) / scale
    print(f"d={d}: against the scale pass {err.max():.2e} (bound 1e-12)")
    assert err.max() <= 1e-12
    assert np.array_equal(ds._column_moments_multi(w[None, :]), ds._column_moments_multi(w[None, :], np.ones(d), np.zeros((1, d))))


def test_multi_component_sweep_on_an_empty_dataset_and_bad_arguments(P):
    ds = P.Dataset(np.empty((0, 5)))
    assert np.array_equal(ds._column_moments_multi(np.empty((3, 0)), np.ones(5), np.ones((3, 5))), np.zeros((3, 3, 5)))
    full = P.Dataset(np.ones((4, 5)))
    with pytest.raises(ValueError):
        full._column_moments_multi(np.ones((2, 3)))  # one weight per row and component
    with pytest.raises(P.PPCAError):
        full._column_moments_multi(np.ones((17, 4)))  # at most 16 components


# --------------------------------------------------------------------------- llks / llk / infer_cluster against the dense Gaussians
def test_llks_and_cluster_posteriors_against_the_dense_gaussians(P):
    """psi spans 100x across the columns, one row is all masked (llk 0, posterior = the prior weights), the data carries weights."""
    n, d, k, nm = 1500, 64, 5, 3
    psi = np.geomspace(0.05, 5.0, d)[np.random.default_rng(1).permutation(d)]
    x, cs, mus, _ = R.synth(n, d, k, nm, psi, 0.3, 21, separation=0.3, own=0.3)
    x[4] = np.nan
    rng = np.random.default_rng(22)
    w = rng.uniform(0.5, 2.0, n)
    logw = R.log_softmax(rng.standard_normal(nm))
    model = P.FAMix(psi * rng.uniform(0.8, 1.25, d), [c + 0.1 * psi[:, None] * rng.standard_normal((d, k)) for c in cs], mus, logw)
    args = (model.noise, list(model.transforms), list(model.means), model.log_weights)
    ds = P.Dataset(x, w)
    want, want_lp = R.llks(x, *args), R.log_posteriors(x, *args)
    got, got_lp = model.llks(ds), model.infer_cluster(ds)
    err = (np.abs(got - want) / (np.abs(want) + d)).max()
    tot, tot_want = model.llk(ds), float(w @ want)
    err_t = abs(tot - tot_want) / float(w @ (np.abs(want) + d))
    # a log-posterior is a difference of two row log-densities: measured like them; the posteriors themselves absolutely
    comp = R.component_llks(x, *args[:3])
    err_lp = (np.abs(got_lp - want_lp) / (np.abs(comp).max(0) + d)[:, None]).max()
    err_p = np.abs(np.exp(got_lp) - np.exp(want_lp)).max()
    soft = np.mean(np.exp(want_lp).max(1) < 0.99)
    print(f"llks {err:.2e}, llk {err_t:.2e}, log-posteriors {err_lp:.2e}, posteriors {err_p:.2e} (bound {TOL:g}); "
          f"{100 * soft:.0f} % of the rows have no component above 0.99")
    assert got[4] == 0.0 and np.allclose(got_lp[4], model.log_weights, rtol=0, atol=1e-14)
    assert got_lp.shape == (n, nm)
    assert max(err, err_t, err_lp, err_p) <= TOL


# --------------------------------------------------------------------------- iterate against the restatement
# (separation of the means, share of each component's own loadings: components that overlap, so that the responsibilities are soft)
ITER_SHAPES = [(3000, 256, 10, 3, 0.1, 0.1), (2000, 200, 16, 2, 0.1, 0.1), (1200, 64, 20, 2, 0.3, 0.3), (1500, 300, 4, 3, 0.1, 0.1)]


def _iterate_case(P, n, d, k, nm, sep, own, spread=10.0):
    rng = np.random.default_rng(40 + d)
    psi_true = np.geomspace(0.3, 0.3 * spread, d)[rng.permutation(d)]
    x, cs_true, mus_true, _ = R.synth(n, d, k, nm, psi_true, 0.3, 41 + d, separation=sep, own=own)
    x[6] = np.nan
    w = rng.uniform(0.5, 2.0, n)
    w[8] = 0.0
    psi = psi_true * rng.uniform(0.7, 1.4, d)
    cs = [c + 0.05 * psi_true[:, None] * rng.standard_normal((d, k)) for c in cs_true]
    mus = [m + 0.05 * psi_true * rng.standard_normal(d) for m in mus_true]
    return x, w, P.FAMix(psi, cs, mus, rng.standard_normal(nm))


@pytest.mark.parametrize("n,d,k,nm,sep,own", ITER_SHAPES, ids=["fused", "two-kernel", "split-k20", "split-d300"])
def test_iterate_against_the_restatement(P, n, d, k, nm, sep, own):
    """30 % masking, weights, a zero-weight row, an all-masked row; signal variance at most 9 psi_j^2 per column.  The returned llk is
    the input model's: against the restatement and against llk(), both to 1e-10 of |llk|."""
    x, w, model = _iterate_case(P, n, d, k, nm, sep, own)
    ds = P.Dataset(x, w)
    resp = R.responsibilities(x, model.noise, list(model.transforms), list(model.means), model.log_weights)[1]
    soft = float(np.mean(resp.max(1) < 0.99))
    assert 0.05 < soft < 0.95  # (rows that keep weight in several components AND rows that one component owns)
    assert P._lib.lib().ppca_path_kind(d, k) == (1 if (d <= 256 and k <= 10) else 0)
    new, llk = model.iterate_with_llk(ds)
    *want, llk_ref = R.iterate(x, w, model.noise, list(model.transforms), list(model.means), model.log_weights)
    errs = _mix_errors(new, want)
    llk_pass = model.llk(ds)
    print(f"({n}, {d}, {k}, K={nm}), {100 * soft:.0f} % soft rows: psi {errs[0]:.2e}, C {errs[1]:.2e}, mean {errs[2]:.2e}, log-weights {errs[3]:.2e} (bound {TOL:g}); "
          f"llk vs restatement {abs(llk - llk_ref) / abs(llk_ref):.2e}, vs llk() {abs(llk - llk_pass) / abs(llk_ref):.2e} (bound 1e-10)")
    assert max(errs) <= TOL
    assert abs(llk - llk_ref) <= 1e-10 * abs(llk_ref) and abs(llk - llk_pass) <= 1e-10 * abs(llk_ref)
    plain = model.iterate(ds)
    assert all(np.array_equal(getattr(plain, f), getattr(new, f)) for f in ("noise", "transforms", "means", "log_weights"))
    floor = np.zeros(d)
    floor[1] = 2.0 * new.noise[1]
    bound = model.iterate(ds, min_noise=floor)
    assert bound.noise[1] == floor[1] and np.array_equal(np.delete(bound.noise, 1), np.delete(new.noise, 1))


# --------------------------------------------------------------------------- properties that need no restatement
def _truth(P, d, k, nm, spread, seed, sep=1.0):
    rng = np.random.default_rng(seed)
    psi = np.geomspace(1.0, spread, d)[rng.permutation(d)]
    return P.FAMix(psi, psi[None, :, None] * rng.standard_normal((nm, d, k)), psi * (rng.standard_normal(d) + sep * rng.standard_normal((nm, d))),
                   0.3 * rng.standard_normal(nm))


def test_one_component_is_the_factor_analysis_step(P):
    n, d, k = 1500, 64, 5
    x, w, mix = _iterate_case(P, n, d, k, 1, 0.0, 1.0)
    ds = P.Dataset(x, w)
    fa = P.FAModel(mix.noise, mix.transforms[0], mix.means[0])
    new, llk = mix.iterate_with_llk(ds)
    want, llk_fa = fa.iterate_with_llk(ds)
    e_psi = np.abs(new.noise / want.noise - 1).max()
    e_c = np.abs(new.transforms[0] - want.transform).max() / np.abs(want.transform).max()
    e_m = (np.abs(new.means[0] - want.mean) / np.maximum(np.abs(want.mean), want.noise)).max()
    print(f"K = 1 against FAModel.iterate: psi {e_psi:.2e}, C {e_c:.2e}, mean {e_m:.2e}, llk {abs(llk - llk_fa) / abs(llk_fa):.2e} (bound 1e-10)")
    assert max(e_psi, e_c, e_m) <= 1e-10 and abs(llk - llk_fa) <= 1e-10 * abs(llk_fa)
    assert new.log_weights.shape == (1,) and abs(new.log_weights[0]) <= 1e-15


def test_iterate_commutes_with_rescaling_columns(P):
    n, d, k, nm = 2000, 64, 5, 2
    x, w, m = _iterate_case(P, n, d, k, nm, 0.3, 0.3, spread=5.0)
    g = np.ones(d)
    g[3], g[10] = 1e3, 1e-3
    ms = P.FAMix(m.noise * g, m.transforms * g[None, :, None], m.means * g, m.log_weights)
    ds, dss = P.Dataset(x, w), P.Dataset(x * g, w)
    new, llk = m.iterate_with_llk(ds)
    news, llks = ms.iterate_with_llk(dss)
    back = P.FAMix(news.noise / g, news.transforms / g[None, :, None], news.means / g, news.log_weights)
    errs = _mix_errors(back, (new.noise, list(new.transforms), list(new.means), new.log_weights))
    shift = float(ds.column_stats()[0] @ np.log(g))
    print(f"rescaled step: psi {errs[0]:.2e}, C {errs[1]:.2e}, mean {errs[2]:.2e}, log-weights {errs[3]:.2e}; "
          f"llk shift {abs(llks - (llk - shift)) / abs(llk):.2e} (bound 1e-9)")
    assert max(errs) <= 1e-9
    assert abs(llks - (llk - shift)) <= 1e-9 * abs(llk)


def test_llk_never_decreases(P):
    """An ECM step cannot lower the log-likelihood: 25 iterations from a random start, each llk >= the previous - 1e-9 |llk|."""
    ds = _truth(P, 64, 5, 3, 15.0, 51).sample(20000, 0.3, seed=52)
    model, llks = P.FAMix.init(3, 5, ds, seed=53), []
    for _ in range(25):
        model, llk = model.iterate_with_llk(ds)
        llks.append(llk)
    llks.append(model.llk(ds))
    steps = np.diff(llks)
    print(f"llk {llks[0]:.6e} -> {llks[-1]:.6e}; smallest step {steps.min():.3e}")
    assert np.all(steps >= -1e-9 * np.abs(llks[:-1]))
    assert llks[-1] > llks[0]


def test_smooth_and_extrapolate(P):
    n, d, k, nm = 1500, 200, 6, 2
    truth = _truth(P, d, k, nm, 20.0, 71, sep=0.15)
    ds = truth.sample(n, 0.3, seed=72).with_weights(np.random.default_rng(73).uniform(0.5, 2.0, n))
    x = ds.numpy()
    want = R.smooth(x, truth.noise, list(truth.transforms), list(truth.means), truth.log_weights)
    sm = truth.smooth(ds).numpy()
    obs = np.isfinite(x)
    err = (np.abs(sm - want) / truth.noise).max()  # every entry against its column's noise level psi_j
    ex = truth.extrapolate(ds)
    e = ex.numpy()
    err_x = (np.abs(e - want) / truth.noise)[~obs].max()
    print(f"smooth {err:.2e}, extrapolate on masked entries {err_x:.2e}, both in units of psi_j (bound {TOL:g})")
    assert err <= TOL and err_x <= TOL
    assert np.array_equal(e[obs], x[obs])  # observed entries bit for bit
    assert np.array_equal(ex.weights(), ds.weights())


def test_trainer_beats_the_isotropic_mixture_on_heteroscedastic_clusters(P, capsys):
    """The model class earns its keep: on data from an FA mixture whose noise levels span 30x, from the same seed and after the same
    number of iterations, FAMixTrainer's log-likelihood per sample is above PPCAMixTrainer's.  A sanity check of the whole loop."""
    n, d, k, nm = 50_000, 32, 4, 3
    truth = _truth(P, d, k, nm, 30.0, 81)
    ds = truth.sample(n, 0.3, seed=82)
    fa = P.FAMixTrainer(ds).train(n_models=nm, state_size=k, n_iters=20, quiet=True, seed=83)
    pp = P.PPCAMixTrainer(ds).train(n_models=nm, state_size=k, n_iters=20, quiet=True, seed=83)
    assert isinstance(fa, P.FAMix) and fa.n_models == nm
    llk_fa, llk_pp, llk_truth = fa.llk(ds), pp.llk(ds), truth.llk(ds)
    with capsys.disabled():
        print(f"\nper-sample llk: FAMix {llk_fa / n:.4f}, PPCAMix {llk_pp / n:.4f}, generating model {llk_truth / n:.4f}")
    assert llk_fa > llk_pp
    assert np.all(fa.noise >= 1e-3 * np.sqrt(ds.column_stats()[2]))
    noisy = P.FAMixTrainer(ds).train(n_models=nm, state_size=k, n_iters=1, seed=83)  # the metric line of the loop
    assert "Masked FA mix iteration 1: aic=" in capsys.readouterr().out and isinstance(noisy, P.FAMix)
