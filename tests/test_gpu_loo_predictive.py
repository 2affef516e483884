"""The leave-one-out predictive of every entry on the GPU (PPCAModel.loo_predictive / loo_llks / loo_llk and the same on PPCAMix):
against the CPU oracle by brute force -- one copy of a row per observed entry with that entry masked, then the oracle's extrapolate,
extrapolated covariance diagonal and llks difference -- and against the closed form of DESIGN.md 4.10 restated in numpy from the
oracle's posteriors for every row."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(3000, 256, 10), (600, 31, 6), (2000, 200, 16), (1500, 300, 4), (400, 160, 100)]
LOG_2PI = np.log(2.0 * np.pi)
TOL_MV = 1e-8  # means and variances, of the predictive's scale, where the oracle's leverage is <= 0.99
TOL_L = 1e-7  # log-densities, absolute (per observed entry for llks)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _data(n, d, seed, mask=0.3):
    rng = np.random.default_rng(seed)
    kt = min(5, d)
    x = rng.standard_normal((n, kt)) @ rng.standard_normal((kt, d)) + 0.3 * rng.standard_normal((n, d)) + rng.standard_normal(d)
    x[rng.random((n, d)) < mask] = np.nan
    if n > 10:
        x[3] = np.nan  # all masked
        x[5] = np.nan
        x[5, d // 2] = 1.5  # one observed entry
        x[7] = rng.standard_normal(d)  # fully observed
        x[1, min(2, d - 1)] = np.inf  # masked as everywhere else
    return x, rng.uniform(0.5, 2.0, n)


def _model(rng, d, k):
    return 0.9, 0.5 * rng.standard_normal((d, k)), 0.3 * rng.standard_normal(d)


def _closed_form(x, s, c, mu, states, covs):
    """DESIGN.md 4.10 from the posterior (states, covs): mean, variance, l per entry (l = 0 on masked entries), leverage."""
    s2 = s * s
    ob = np.isfinite(x)
    pm = states @ c.T + mu
    q = np.einsum("ja,nab,jb->nj", c, covs, c)
    vp = s2 + (c * c).sum(axis=1)
    sj = s2 - q
    xo = np.where(ob, x, 0.0)
    r = xo - pm
    prior = ~(sj * vp > s2 * s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mo, vo = xo - s2 * r / sj, s2 * s2 / sj
        lo = -0.5 * (LOG_2PI + np.log(vo) + r * r / sj)
    lpr = -0.5 * (LOG_2PI + np.log(vp) + (xo - mu) ** 2 / vp)
    mean = np.where(ob, np.where(prior, mu, mo), pm)
    var = np.where(ob, np.where(prior, vp, vo), s2 + q)
    ell = np.where(ob, np.where(prior, lpr, lo), 0.0)
    return mean, var, ell, q / s2


def _masked_copies(x, rows):
    reps, ii, jj = [], [], []
    for i in rows:
        for j in np.flatnonzero(np.isfinite(x[i])):
            xm = x[i].copy()
            xm[j] = np.nan
            reps.append(xm)
            ii.append(i)
            jj.append(j)
    return np.array(reps), np.array(ii, dtype=np.int64), np.array(jj, dtype=np.int64)


def _brute(oracle, x, s, c, mu, rows):
    """Per observed entry (i, j) of the rows: the oracle's extrapolated value and covariance diagonal of the row with j masked,
    and llks(row) - llks(row with j masked)."""
    xm, ii, jj = _masked_copies(x, rows)
    t = np.arange(len(ii))
    ext = oracle.reconstruct(xm, s, c, mu, "extrapolate")[t, jj]
    cd = oracle.covariance_diagonal(xm, s, c, mu, "extrapolate")[t, jj]
    full = dict(zip(rows, oracle.llks(x[rows], s, c, mu)))
    ell = np.array([full[i] for i in ii]) - oracle.llks(xm, s, c, mu)
    return ii, jj, ext, cd, ell


def _close(got, want, scale, tol):
    err = np.abs(got - want) / scale
    assert np.all(err <= tol), (err.max(), np.argmax(err))


def _spread(n, count=80):
    return np.unique(np.linspace(0, n - 1, min(count, n)).astype(np.int64))


def _dev_extrapolated(P, m, ds):
    from ppca_rs_amd import _lib

    h = C.c_void_p()
    _lib.check(_lib.lib().ppca_covariance_diagonal(ds._ctx.handle, ds._h, m._device(ds._ctx).h, 1, C.byref(h)))
    return m.extrapolate(ds).numpy(), P.Dataset._wrap(h, ds._ctx).numpy()


# ------------------------------------------------------------------ 1. the oracle, both paths
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_loo_matches_the_oracle(P, oracle, n, d, k):
    rng = np.random.default_rng(n + 7 * d + k)
    x, w = _data(n, d, d + k)
    s, c, mu = _model(rng, d, k)
    xn = np.where(np.isfinite(x), x, np.nan)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    res = m.loo_predictive(ds)
    mean, var, llks = res.mean().numpy(), res.variance().numpy(), res.llks()
    assert mean.shape == (n, d) and np.all(np.isfinite(mean)) and np.all(var > 0)
    ob = np.isfinite(xn)
    states, covs = oracle.infer(xn, s, c, mu)
    cm, cv, cl, lev = _closed_form(xn, s, c, mu, states, covs)
    ok = ~ob | (lev <= 0.99)
    scale = np.maximum(np.abs(cm), np.sqrt(cv))
    _close(mean[ok], cm[ok], scale[ok], TOL_MV)
    _close(var[ok], cv[ok], cv[ok], TOL_MV)
    nobs = ob.sum(axis=1)
    _close(llks, cl.sum(axis=1), np.maximum(nobs, 1), TOL_L)
    assert llks[3] == 0.0
    # brute force on a spread of rows across many tiles
    rows = np.union1d(_spread(n), [3, 5, 7])
    ii, jj, ext, cd, ell = _brute(oracle, xn, s, c, mu, rows)
    sel = lev[ii, jj] <= 0.99
    assert sel.mean() > 0.5
    g_m, g_v = mean[ii, jj][sel], var[ii, jj][sel]
    _close(g_m, ext[sel], np.maximum(np.abs(ext[sel]), np.sqrt(cd[sel])), TOL_MV)
    _close(g_v, cd[sel], cd[sel], TOL_MV)
    _close(cl[ii, jj][sel], ell[sel], 1.0, TOL_L)
    # the per-row sums of the brute-force l
    per = np.zeros(n)
    np.add.at(per, ii, ell)
    _close(llks[rows], per[rows], np.maximum(nobs[rows], 1), TOL_L)
    # masked entries: what extrapolate and the extrapolated covariance diagonal give
    e_m, e_v = _dev_extrapolated(P, m, ds)
    _close(mean[~ob], e_m[~ob], np.maximum(np.abs(e_m[~ob]), np.sqrt(e_v[~ob])), 1e-10)
    _close(var[~ob], e_v[~ob], e_v[~ob], 1e-10)
    # weights: carried, and llk = sum w llks
    assert np.array_equal(res.mean().weights(), w) and np.array_equal(res.variance().weights(), w)
    assert abs(res.llk() - np.dot(w, llks)) <= 1e-12 * np.abs(w * llks).sum()
    # the llks-only calls
    only = m.loo_llks(ds)
    assert np.all(np.abs(only - llks) <= 1e-14 * np.abs(llks))
    assert abs(m.loo_llk(ds) - res.llk()) <= 1e-14 * abs(res.llk())
    # z-scores
    z = res.zscores()
    assert np.all(np.isnan(z[~ob])) and np.all(np.isfinite(z[ob]))
    _close(z[ob], ((xn - mean) / np.sqrt(var))[ob], 1.0, 1e-12)


# ------------------------------------------------------------------ 2. edge cases
@pytest.mark.parametrize("d,k", [(64, 5), (300, 6)])
def test_edge_rows(P, oracle, d, k):
    rng = np.random.default_rng(d + k)
    s, c, mu = _model(rng, d, k)
    m = P.PPCAModel(s, c, mu)
    prior_v = s * s + (c * c).sum(axis=1)
    x = rng.standard_normal((3, d))
    x[0] = np.nan  # all masked: (mu, sigma^2 + |c_j|^2)
    x[1] = np.nan
    x[1, 4] = 0.7  # one observed entry: the prior predictive for it too
    res = m.loo_predictive(P.Dataset(x))
    mean, var, llks = res.mean().numpy(), res.variance().numpy(), res.llks()
    _close(mean[0], mu, np.sqrt(prior_v), 1e-12)
    _close(var[0], prior_v, prior_v, 1e-12)
    _close(mean[1, 4], mu[4], np.sqrt(prior_v[4]), 1e-12)
    _close(var[1, 4], prior_v[4], prior_v[4], 1e-12)
    assert llks[0] == 0.0
    want = -0.5 * (LOG_2PI + np.log(prior_v[4]) + (0.7 - mu[4]) ** 2 / prior_v[4])
    assert abs(llks[1] - want) < 1e-10
    # fully observed row (2): the brute force
    ii, jj, ext, cd, ell = _brute(oracle, x, s, c, mu, [2])
    _close(mean[2, jj], ext, np.maximum(np.abs(ext), np.sqrt(cd)), TOL_MV)
    _close(var[2, jj], cd, cd, TOL_MV)
    assert abs(llks[2] - ell.sum()) < TOL_L * d
    # one row alone = that row of the whole
    one = m.loo_predictive(P.Dataset(x[2:3]))
    _close(one.mean().numpy()[0], mean[2], np.maximum(np.abs(mean[2]), 1.0), 1e-12)
    _close(one.llks(), llks[2:3], abs(llks[2]), 1e-12)


def test_state_size_zero_and_empty(P):
    rng = np.random.default_rng(3)
    d, s = 40, 0.8
    mu = rng.standard_normal(d)
    m = P.PPCAModel(s, np.zeros((d, 0)), mu)
    x, w = _data(200, d, 11)
    res = m.loo_predictive(P.Dataset(x, w))
    ob = np.isfinite(x)
    _close(res.mean().numpy(), np.tile(mu, (200, 1)), np.maximum(np.abs(mu), 1.0), 1e-14)
    _close(res.variance().numpy(), np.full((200, d), s * s), s * s, 1e-14)
    want = np.where(ob, -0.5 * (LOG_2PI + np.log(s * s) + (np.where(ob, x, 0) - mu) ** 2 / (s * s)), 0.0).sum(axis=1)
    _close(res.llks(), want, np.maximum(ob.sum(axis=1), 1), 1e-12)
    # an empty dataset
    rng2 = np.random.default_rng(4)
    s1, c1, mu1 = _model(rng2, d, 4)
    for mm in (m, P.PPCAModel(s1, c1, mu1)):
        e = mm.loo_predictive(P.Dataset(np.empty((0, d))))
        assert e.mean().numpy().shape == (0, d) and e.variance().numpy().shape == (0, d)
        assert e.llks().shape == (0,) and e.llk() == 0.0
        assert mm.loo_llk(P.Dataset(np.empty((0, d)))) == 0.0


def test_no_output_is_an_error(P):
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(5)
    s, c, mu = _model(rng, 16, 3)
    m, ds = P.PPCAModel(s, c, mu), P.Dataset(rng.standard_normal((10, 16)))
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_loo_predictive(ds._ctx.handle, ds._h, m._device(ds._ctx).h, None, None, None, None))


# ------------------------------------------------------------------ 3. the Gram guard's fallback and the s_j <= 0 rule
def test_guard_tripping_model(P, oracle):
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(77)
    n, d, k = 1000, 256, 10
    x, w = _data(n, d, 8)
    s, c, mu = _model(rng, d, k)
    c[0] *= 1e8  # rows of C spanning 1e8: the int8 Gram's guard trips
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    eng = C.c_int32(-1)
    _lib.check(_lib.lib().ppca_gram_engine(ds._ctx.handle, m._device(ds._ctx).h, C.byref(eng)))
    assert eng.value == 1
    xn = np.where(np.isfinite(x), x, np.nan)
    res = m.loo_predictive(ds)
    mean, var, llks = res.mean().numpy(), res.variance().numpy(), res.llks()
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(var > 0) and np.all(np.isfinite(llks))
    # rows that do not observe dimension 0: the oracle
    free = np.flatnonzero(~np.isfinite(xn[:, 0]))
    assert len(free) > 200
    rows = free[_spread(len(free), 64)]
    states, covs = oracle.infer(xn[rows], s, c, mu)
    cm, cv, cl, lev = _closed_form(xn[rows], s, c, mu, states, covs)
    ok = ~np.isfinite(xn[rows]) | (lev <= 0.99)
    _close(mean[rows][ok], cm[ok], np.maximum(np.abs(cm), np.sqrt(cv))[ok], TOL_MV)
    _close(var[rows][ok], cv[ok], cv[ok], TOL_MV)
    _close(llks[rows], cl.sum(axis=1), np.maximum(np.isfinite(xn[rows]).sum(axis=1), 1), TOL_L)
    # rows that observe it: dimension 0 alone pins a latent direction (h_0 -> 1); its predictive is at most the prior's
    seen = np.flatnonzero(np.isfinite(xn[:, 0]))
    prior_v0 = s * s + (c[0] ** 2).sum()
    assert np.all(var[seen, 0] <= prior_v0 * (1 + 1e-12))


# ------------------------------------------------------------------ 4. independence of the grid, the chunking and the split
@pytest.mark.parametrize("n,d,k", [(20000, 256, 10), (3000, 300, 4)])
def test_grid_chunks_and_slices(P, monkeypatch, n, d, k):
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(5 + k)
    x, w = _data(n, d, 40 + k)
    s, c, mu = _model(rng, d, k)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    base = m.loo_predictive(ds)
    bm, bv, bl = base.mean().numpy(), base.variance().numpy(), base.llks()
    again = m.loo_predictive(ds)
    assert np.array_equal(again.mean().numpy(), bm) and np.array_equal(again.llks(), bl)  # deterministic

    def same(r, tol=1e-12):
        _close(r.mean().numpy(), bm, np.maximum(np.abs(bm), 1.0), tol)
        _close(r.variance().numpy(), bv, bv, tol)
        _close(r.llks(), bl, np.maximum(np.abs(bl), 1.0), tol)

    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(3)  # a few workgroups, hundreds of tiles / rows each
        same(m.loo_predictive(ds))
    finally:
        ctx.set_grid_limit(0)
    monkeypatch.setenv("PPCA_GEN_CHUNK", "256")  # the split pipeline in several chunks
    same(m.loo_predictive(ds))
    monkeypatch.delenv("PPCA_GEN_CHUNK")
    s0, ln = n // 3 + 5, n // 4
    part = m.loo_predictive(ds._slice(s0, ln))
    _close(part.mean().numpy(), bm[s0:s0 + ln], np.maximum(np.abs(bm[s0:s0 + ln]), 1.0), 1e-12)
    _close(part.variance().numpy(), bv[s0:s0 + ln], bv[s0:s0 + ln], 1e-12)
    _close(part.llks(), bl[s0:s0 + ln], np.maximum(np.abs(bl[s0:s0 + ln]), 1.0), 1e-12)


def test_outputs_do_not_depend_on_the_row_chunks(P, monkeypatch):
    """PPCA_POST_CHUNK=64 at n = 150: three chunks of the posterior scratch, the last of 22 rows, against one chunk -- bit for bit.
    The mixture with the variance takes both sweeps over its components (k = 2 and k = 3) in every chunk."""
    n, d, k = 150, 13, 3
    rng = np.random.default_rng(61)
    x, w = _data(n, d, 62)
    s, c, mu = _model(rng, d, k)
    ds = P.Dataset(x, w)
    m = P.PPCAModel(s, c, mu)
    mix = P.PPCAMix([P.PPCAModel(0.8, 0.5 * rng.standard_normal((d, 2)), 0.3 * rng.standard_normal(d)), m], np.log([0.4, 0.6]))

    def outputs():
        got = []
        for model in (m, mix):
            r = model.loo_predictive(ds)
            got += [r.mean().numpy(), r.variance().numpy(), r.llks()]
        return got

    base = outputs()
    monkeypatch.setenv("PPCA_POST_CHUNK", "64")
    chunked = outputs()
    monkeypatch.delenv("PPCA_POST_CHUNK")
    for name, a, b in zip(("mean", "variance", "llks", "mix mean", "mix variance", "mix llks"), chunked, base):
        assert np.array_equal(a, b), (name, np.argwhere(a != b)[:8])


# ------------------------------------------------------------------ 5. mixture
def _pad(cs, kmax):
    return np.stack([np.concatenate([c_, np.zeros((c_.shape[0], kmax - c_.shape[1]))], axis=1) for c_ in cs])


@pytest.mark.parametrize("d,ks", [(20, (3, 5, 2)), (300, (4, 6))])
def test_mixture_matches_the_oracle(P, oracle, d, ks):
    rng = np.random.default_rng(19 + d)
    nm = len(ks)
    n = 600
    x = np.concatenate([oracle.synth(n // nm, d, 3, 0.3, 500 + c_ + d, mean_scale=2.0)[0] for c_ in range(nm)])
    n = x.shape[0]
    x[7] = np.nan
    x[9] = np.nan
    x[9, 1] = 0.4
    w = rng.uniform(0.5, 2.0, n)
    sig = np.array([0.8, 1.1, 0.6])[:nm]
    cs = [rng.standard_normal((d, k_)) for k_ in ks]
    ms = rng.standard_normal((nm, d))
    lw = np.log(np.array([0.5, 0.2, 0.3])[:nm] / np.array([0.5, 0.2, 0.3])[:nm].sum())
    ds = P.Dataset(x, w)
    mix = P.PPCAMix([P.PPCAModel(sig[c_], cs[c_], ms[c_]) for c_ in range(nm)], lw)
    res = mix.loo_predictive(ds)
    mean, var, llks = res.mean().numpy(), res.variance().numpy(), res.llks()
    assert np.all(np.isfinite(mean)) and np.all(var > 0)
    assert np.array_equal(res.mean().weights(), np.ones(n))  # no weights, like every mixture output
    ob = np.isfinite(x)
    cpad = _pad(cs, max(ks))
    rows = np.union1d(_spread(n, 64), [7, 9])
    xm, ii, jj = _masked_copies(x, rows)
    t = np.arange(len(ii))
    inf = oracle.mix_inferred(xm, sig, cpad, ms, lw)
    ext, cd = inf["extrapolate"][t, jj], inf["extrapolate_covariance_diagonal"][t, jj]
    full = dict(zip(rows, oracle.mix_llks(x[rows], sig, cpad, ms, lw)))
    ell = np.array([full[i] for i in ii]) - oracle.mix_llks(xm, sig, cpad, ms, lw)
    _close(mean[ii, jj], ext, np.maximum(np.abs(ext), np.sqrt(cd)), TOL_MV)
    _close(var[ii, jj], cd, cd, TOL_MV)
    per = np.zeros(n)
    np.add.at(per, ii, ell)
    _close(llks[rows], per[rows], np.maximum(ob[rows].sum(axis=1), 1), TOL_L)
    assert llks[7] == 0.0
    # masked entries: PPCAMix.extrapolate and the extrapolated covariance diagonal around it
    from ppca_rs_amd import _lib

    devs, arr = mix._handles(ds._ctx)
    h = C.c_void_p()
    _lib.check(_lib.lib().ppca_mix_reconstruct(ds._ctx.handle, ds._h, arr, _lib.ptr(mix._lw), nm, 3, C.byref(h)))
    e_v = P.Dataset._wrap(h, ds._ctx).numpy()
    e_m = mix.extrapolate(ds).numpy()
    _close(mean[~ob], e_m[~ob], np.maximum(np.abs(e_m[~ob]), np.sqrt(e_v[~ob])), 1e-10)
    _close(var[~ob], e_v[~ob], e_v[~ob], 1e-10)
    # totals and the llks-only calls
    assert abs(res.llk() - np.dot(w, llks)) <= 1e-12 * np.abs(w * llks).sum()
    assert np.all(np.abs(mix.loo_llks(ds) - llks) <= 1e-14 * np.abs(llks))
    assert abs(mix.loo_llk(ds) - res.llk()) <= 1e-14 * abs(res.llk())


def test_one_component_mixture_is_the_model(P):
    rng = np.random.default_rng(23)
    for d, k in ((64, 5), (300, 6)):
        x, w = _data(500, d, 2 + d)
        s, c, mu = _model(rng, d, k)
        ds = P.Dataset(x, w)
        a = P.PPCAModel(s, c, mu).loo_predictive(ds)
        b = P.PPCAMix([P.PPCAModel(s, c, mu)], np.zeros(1)).loo_predictive(ds)
        am = a.mean().numpy()
        _close(b.mean().numpy(), am, np.maximum(np.abs(am), 1.0), 1e-12)
        _close(b.variance().numpy(), a.variance().numpy(), a.variance().numpy(), 1e-12)
        _close(b.llks(), a.llks(), np.maximum(np.abs(a.llks()), 1.0), 1e-12)
