"""Masked factor analysis (per-column noise) on the GPU: the streaming scale pass against numpy, FAModel's llks / iterate against the
dense restatement in original units (tests/fa_restatement.py), and the properties the model adds over PPCAModel -- a log-likelihood
that never decreases, and EM steps that commute with rescaling columns.

Tolerance: the project's GPU parity tolerance, 1e-5 relative (psi per element; C against max |C|; mean_j against max(|mean_j|, psi_j);
a row's llk against |llk| + d), unless a check says exact.  Each parity check prints its worst error before asserting."""
import numpy as np
import pytest

import fa_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _model_errors(got, want):
    (p1, c1, m1), (p0, c0, m0) = got, want
    return (np.abs(p1 / p0 - 1).max(), np.abs(c1 - c0).max() / np.abs(c0).max(), (np.abs(m1 - m0) / np.maximum(np.abs(m0), p0)).max())


def _arrays(m):
    return m.noise, m.transform, m.mean


# --------------------------------------------------------------------------- the pass against numpy
N_PASS = 3001


def _pass_inputs(d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N_PASS + 40, d)) * rng.uniform(0.1, 10.0, d) + rng.standard_normal(d)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[9] = np.nan  # an all-masked row
    x[11, d // 2] = np.inf  # masked like every non-finite entry
    x[:, d - 1] = np.where(np.arange(x.shape[0]) % 97 == 0, x[:, d - 1], np.nan)  # a nearly empty column
    w = rng.uniform(0.5, 2.0, x.shape[0])
    a = rng.uniform(0.2, 5.0, d) * rng.choice([-1.0, 1.0], d)
    return x, w, a, rng.standard_normal(d), rng.standard_normal(d)


def _pass_reference(x, w, a, b, l):
    obs = np.isfinite(x)
    y = x * a
    e = np.where(obs, y - b, 0.0)
    wm = w[:, None] * obs
    sums = np.stack([wm.sum(0), (wm * e).sum(0), (wm * e * e).sum(0)])
    scale = np.stack([sums[0], (wm * np.abs(e)).sum(0), sums[2]])  # what each column sum is a sum OF: the measure of its rounding
    lo = np.where(obs, l, 0.0)
    return obs, y, sums, scale, lo.sum(1), np.abs(lo).sum(1)


@pytest.mark.parametrize("weighted,sliced", [(False, False), (True, True)], ids=["plain", "weighted-slice"])
@pytest.mark.parametrize("d", [256, 200, 1024, 7])
def test_scale_pass_against_numpy(P, d, weighted, sliced):
    x, w, a, b, l = _pass_inputs(d, 100 + d)
    lo = 23 if sliced else 0  # (an odd first row: with d = 7 the slice's rows are not 16-byte aligned)
    full = P.Dataset(x, w if weighted else None)
    ds = full._slice(lo, N_PASS) if sliced else P.Dataset(np.ascontiguousarray(x[:N_PASS]), w[:N_PASS] if weighted else None)
    xs, ws = x[lo:lo + N_PASS], (w[lo:lo + N_PASS] if weighted else np.ones(N_PASS))
    obs, y, sums, scale, rows, rows_scale = _pass_reference(xs, ws, a, b, l)

    out, got_sums, got_rows = ds._scale_columns(a, b, l, col_sums=True, row_sums=True)
    o = out.numpy()
    assert np.array_equal(o[obs], y[obs]) and np.isnan(o[~obs]).all()  # x * a bit for bit; NaN on masked entries
    assert np.array_equal(out.weights(), ws)
    err_c = np.abs(got_sums - sums) / np.where(scale > 0, scale, 1.0)
    err_r = np.abs(got_rows - rows) / np.where(rows_scale > 0, rows_scale, 1.0)
    print(f"d={d}: column sums {err_c.max():.2e}, row sums {err_r.max():.2e} (bound 1e-12)")
    assert err_c.max() <= 1e-12 and err_r.max() <= 1e-12
    assert np.all(got_sums[:, scale[0] == 0] == 0.0) and np.all(got_rows[~obs.any(1)] == 0.0)

    # two runs are bit-identical; the sums-only form gives the same sums; every output is nullable
    out2, sums2, rows2 = ds._scale_columns(a, b, l, col_sums=True, row_sums=True)
    assert np.array_equal(out2.numpy(), o, equal_nan=True) and np.array_equal(sums2, got_sums) and np.array_equal(rows2, got_rows)
    none, sums3, rows3 = ds._scale_columns(a, b, l, out=False, col_sums=True, row_sums=True)
    assert none is None and np.array_equal(sums3, got_sums) and np.array_equal(rows3, got_rows)
    assert np.array_equal(ds._scale_columns(a, b, l, out=False, col_sums=True)[1], got_sums)
    assert np.array_equal(ds._scale_columns(a, out=False, col_sums=True)[1][0], got_sums[0])  # b, l nullable

    # under a capped grid: out and the row sums unchanged bit for bit, the column sums to 1e-12
    ctx = ds._ctx
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            out_g, sums_g, rows_g = ds._scale_columns(a, b, l, col_sums=True, row_sums=True)
            assert np.array_equal(out_g.numpy(), o, equal_nan=True) and np.array_equal(rows_g, got_rows)
            assert (np.abs(sums_g - sums) / np.where(scale > 0, scale, 1.0)).max() <= 1e-12
    finally:
        ctx.set_grid_limit(0)

    # the fill mode: observed entries as they are, fill * a elsewhere
    fill = np.random.default_rng(d).standard_normal(xs.shape)
    got = ds._fill_masked(P.Dataset(fill), a).numpy()
    assert np.array_equal(got[obs], xs[obs]) and np.array_equal(got[~obs], (fill * a)[~obs])


def test_scale_pass_on_an_empty_dataset(P):
    ds = P.Dataset(np.empty((0, 5)))
    out, sums, rows = ds._scale_columns(np.ones(5), np.ones(5), np.ones(5), col_sums=True, row_sums=True)
    assert len(out) == 0 and out.numpy().shape == (0, 5) and np.array_equal(sums, np.zeros((3, 5))) and rows.shape == (0,)
    assert len(ds._fill_masked(P.Dataset(np.empty((0, 5))), np.ones(5))) == 0
    with pytest.raises(P.PPCAError):
        ds._scale_columns(np.ones(5), out=False)  # no output requested


def test_column_stats_match_numpy(P):
    rng = np.random.default_rng(8)
    n, d = 4001, 37
    x = rng.standard_normal((n, d)) * np.geomspace(1e-2, 1e2, d) + 1e3 * rng.standard_normal(d)  # means far above the spreads
    x[rng.random((n, d)) < 0.4] = np.nan
    x[:, 5] = np.nan
    w = rng.uniform(0.1, 3.0, n)
    tot, mean, var = P.Dataset(x, w).column_stats()
    obs = np.isfinite(x)
    wm = w[:, None] * obs
    t0 = wm.sum(0)
    live = t0 > 0
    m0 = np.where(live, np.nansum(wm * np.where(obs, x, 0.0), 0) / np.where(live, t0, 1), 0.0)
    v0 = np.where(live, (wm * np.where(obs, x - m0, 0.0) ** 2).sum(0) / np.where(live, t0, 1), 0.0)
    assert np.allclose(tot, t0, rtol=1e-12, atol=0) and tot[5] == 0 and mean[5] == 0 and var[5] == 0
    assert np.all(np.abs(mean - m0) <= 1e-12 * (np.abs(m0) + np.sqrt(v0)))
    assert np.all(np.abs(var - v0) <= 1e-10 * v0)


# --------------------------------------------------------------------------- llks / llk against the dense Gaussian
@pytest.mark.parametrize("n,d,k", [(1200, 24, 3), (700, 40, 12)])
def test_llks_against_the_dense_gaussian(P, n, d, k):
    """psi spans 100x across the columns, one row is all masked, the data carries weights."""
    psi = np.geomspace(0.05, 5.0, d)[np.random.default_rng(1).permutation(d)]
    x, c, mu = R.synth(n, d, k, psi, 0.3, 21 + d)
    x[4] = np.nan
    rng = np.random.default_rng(22)
    w = rng.uniform(0.5, 2.0, n)
    model = P.FAModel(psi * rng.uniform(0.8, 1.25, d), c + 0.1 * psi[:, None] * rng.standard_normal((d, k)), mu)
    ds = P.Dataset(x, w)
    want = R.llks(x, *_arrays(model))
    got = model.llks(ds)
    err = (np.abs(got - want) / (np.abs(want) + d)).max()
    tot, tot_want = model.llk(ds), float(w @ want)
    err_t = abs(tot - tot_want) / float(w @ (np.abs(want) + d))
    print(f"({n}, {d}, {k}): llks {err:.2e}, llk {err_t:.2e} (bound {TOL:g})")
    assert got[4] == 0.0
    assert err <= TOL and err_t <= TOL


def test_from_ppca_llks_equal_the_isotropic_models(P):
    rng = np.random.default_rng(31)
    n, d, k = 1500, 48, 6
    x = rng.standard_normal((n, k)) @ rng.standard_normal((k, d)) + 0.7 * rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    ds = P.Dataset(x)
    m = P.PPCAModel(0.7, rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d))
    want, got = m.llks(ds), P.FAModel.from_ppca(m).llks(ds)
    err = (np.abs(got - want) / (np.abs(want) + d)).max()
    print(f"from_ppca llks {err:.2e}")
    assert err <= TOL


# --------------------------------------------------------------------------- iterate against the restatement
ITER_SHAPES = [(3000, 256, 10), (2000, 200, 16), (1500, 300, 4), (1200, 64, 20)]  # fused pass, two-kernel form, split pipeline (d, k)


@pytest.mark.parametrize("n,d,k", ITER_SHAPES)
def test_iterate_against_the_restatement(P, n, d, k):
    """30 % masking, weights, signal variance at most 9 psi_j^2 per column (R.synth): the cancellation in the noise update costs at most
    two digits.  The returned llk is the input model's."""
    rng = np.random.default_rng(40 + d)
    psi_true = np.geomspace(0.3, 3.0, d)[rng.permutation(d)]
    x, c_true, mu_true = R.synth(n, d, k, psi_true, 0.3, 41 + d)
    x[6] = np.nan
    w = rng.uniform(0.5, 2.0, n)
    psi = psi_true * rng.uniform(0.7, 1.4, d)
    c = c_true + 0.2 * psi_true[:, None] * rng.standard_normal((d, k))
    mu = mu_true + 0.3 * psi_true * rng.standard_normal(d)
    model, ds = P.FAModel(psi, c, mu), P.Dataset(x, w)
    assert P._lib.lib().ppca_path_kind(d, k) == (1 if (d <= 256 and k <= 10) else 0)
    new, llk = model.iterate_with_llk(ds)
    want = R.iterate(x, w, psi, c, mu)
    errs = _model_errors(_arrays(new), want)
    ref_llks = R.llks(x, psi, c, mu)
    llk_ref, llk_scale = float(w @ ref_llks), float(w @ (np.abs(ref_llks) + d))
    llk_pass = model.llk(ds)
    print(f"({n}, {d}, {k}): psi {errs[0]:.2e}, C {errs[1]:.2e}, mean {errs[2]:.2e}, llk vs restatement {abs(llk - llk_ref) / llk_scale:.2e}, "
          f"vs llk() {abs(llk - llk_pass) / llk_scale:.2e} (bound {TOL:g})")
    assert max(errs) <= TOL
    assert abs(llk - llk_ref) <= TOL * llk_scale and abs(llk - llk_pass) <= TOL * llk_scale
    plain = model.iterate(ds)
    assert all(np.array_equal(u, v) for u, v in zip(_arrays(plain), _arrays(new)))
    floor = np.zeros(d)
    floor[1] = 2.0 * new.noise[1]
    bound = model.iterate(ds, min_noise=floor)
    assert bound.noise[1] == floor[1] and np.array_equal(np.delete(bound.noise, 1), np.delete(new.noise, 1))


# --------------------------------------------------------------------------- properties that need no restatement
def _truth(P, d, k, spread, seed):
    rng = np.random.default_rng(seed)
    psi = np.geomspace(1.0, spread, d)[rng.permutation(d)]
    return P.FAModel(psi, psi[:, None] * rng.standard_normal((d, k)), psi * rng.standard_normal(d))


def test_llk_never_decreases(P):
    """An ECM step cannot lower the log-likelihood: 25 iterations from a random start, each llk >= the previous - 1e-9 |llk|."""
    ds = _truth(P, 64, 5, 15.0, 51).sample(20000, 0.3, seed=52)
    model, llks = P.FAModel.init(5, ds, seed=53), []
    for _ in range(25):
        model, llk = model.iterate_with_llk(ds)
        llks.append(llk)
    llks.append(model.llk(ds))
    steps = np.diff(llks)
    print(f"llk {llks[0]:.6e} -> {llks[-1]:.6e}; smallest step {steps.min():.3e}")
    assert np.all(steps >= -1e-9 * np.abs(llks[:-1]))
    assert llks[-1] > llks[0]


def test_iterate_commutes_with_rescaling_columns_and_ppca_does_not(P):
    n, d, k = 2000, 32, 4
    truth = _truth(P, d, k, 5.0, 61)
    x = truth.sample(n, 0.3, seed=62).numpy()
    w = np.random.default_rng(63).uniform(0.5, 2.0, n)
    f = np.ones(d)
    f[3], f[10] = 1e3, 1e-3
    rng = np.random.default_rng(64)
    m = P.FAModel(truth.noise * rng.uniform(0.7, 1.4, d), truth.transform + 0.2 * truth.noise[:, None] * rng.standard_normal((d, k)),
                  truth.mean)
    ms = P.FAModel(m.noise * f, m.transform * f[:, None], m.mean * f)
    ds, dss = P.Dataset(x, w), P.Dataset(x * f, w)
    new, llk = m.iterate_with_llk(ds)
    news, llks = ms.iterate_with_llk(dss)
    errs = _model_errors((news.noise / f, news.transform / f[:, None], news.mean / f), _arrays(new))
    tot = ds.column_stats()[0]
    shift = float(tot @ np.log(f))
    print(f"rescaled step: psi {errs[0]:.2e}, C {errs[1]:.2e}, mean {errs[2]:.2e}; llk shift {abs(llks - (llk - shift)) / abs(llk):.2e}")
    assert max(errs) <= TOL
    assert abs(llks - (llk - shift)) <= TOL * abs(llk)
    assert abs(ms.llk(dss) - (m.llk(ds) - shift)) <= TOL * abs(llk)
    # the isotropic model's step does not commute: what the per-column noise adds
    iso = P.PPCAModel(float(np.sqrt(np.mean(m.noise ** 2))), m.transform, m.mean)
    isos = P.PPCAModel(iso.isotropic_noise, iso.transform * f[:, None], iso.mean * f)
    a, b = iso.iterate(ds), isos.iterate(dss)
    gap = np.abs(b.transform / f[:, None] - a.transform).max() / np.abs(a.transform).max()
    print(f"PPCAModel.iterate under the same rescaling: C differs by {gap:.2e} of max |C|")
    assert gap > 1e-2


def test_smooth_extrapolate_and_infer(P):
    n, d, k = 1500, 200, 6
    truth = _truth(P, d, k, 20.0, 71)
    ds = truth.sample(n, 0.3, seed=72).with_weights(np.random.default_rng(73).uniform(0.5, 2.0, n))
    x = ds.numpy()
    inf = truth.infer(ds)
    z = inf.states()
    covs = inf.covariances()
    assert z.shape == (n, k) and len(covs) == n and covs[0].shape == (k, k)
    zr, sr = R.posterior(x[0], *_arrays(truth))
    assert np.abs(z[0] - zr).max() <= TOL * max(1.0, np.abs(zr).max()) and np.abs(covs[0] - sr).max() <= TOL * np.abs(sr).max()
    want = z @ truth.transform.T + truth.mean
    scale = np.abs(want) + truth.noise
    sm = truth.smooth(ds)
    err = (np.abs(sm.numpy() - want) / scale).max()
    print(f"smooth vs C z + mean: {err:.2e}")
    assert err <= TOL and np.array_equal(sm.weights(), ds.weights())
    ex = truth.extrapolate(ds)
    e, obs = ex.numpy(), np.isfinite(x)
    assert np.array_equal(e[obs], x[obs])  # observed entries bit for bit
    assert (np.abs(e - want) / scale)[~obs].max() <= TOL and np.array_equal(ex.weights(), ds.weights())


def test_trainer_beats_ppca_on_heteroscedastic_data(P, capsys):
    """FA nests PPCA, and the noise levels of this data span 30x: from the same start, after the same number of iterations, the FA
    model's log-likelihood is the higher one.  A sanity check of the whole loop, not a tolerance."""
    n, d, k = 200_000, 32, 4
    truth = _truth(P, d, k, 30.0, 81)
    ds = truth.sample(n, 0.3, seed=82)
    fa = P.FATrainer(ds).train(state_size=k, n_iters=30, quiet=True, seed=83)
    pp = P.PPCATrainer(ds).train(state_size=k, n_iters=30, quiet=True, seed=83)
    assert isinstance(fa, P.FAModel)
    llk_fa, llk_pp, llk_truth = fa.llk(ds), pp.llk(ds), truth.llk(ds)
    with capsys.disabled():
        print(f"\nper-sample llk: FA {llk_fa / n:.4f}, PPCA {llk_pp / n:.4f}, generating model {llk_truth / n:.4f}")
    assert llk_fa > llk_pp
    floor = 1e-3 * np.sqrt(ds.column_stats()[2])
    assert np.all(fa.noise >= floor)
    noisy = P.FATrainer(ds).train(state_size=k, n_iters=1, seed=83)  # the metric line of the loop
    assert "Masked FA iteration 1: aic=" in capsys.readouterr().out and isinstance(noisy, P.FAModel)
