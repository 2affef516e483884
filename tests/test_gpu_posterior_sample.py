"""Posterior sampling and multiple imputation on the GPU (PPCAModel.sample_posterior, PPCAMix.sample_posterior): the draw
restated in numpy -- the posterior from the CPU oracle, U by reverse-order Cholesky, the counter-based generator bit for bit
in uint64 -- and its independence of the grid, the path, the chunking and the split of the rows.

The normals are computed in fp32 on the device and in fp64 here from the same 24-bit uniforms: they agree to a few fp32
ulps (relative 1e-6 at the worst), so the draws are compared at 1e-5 of the row's scale."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5  # of the row's scale: fp32 Box-Muller
SHAPES = [(3000, 256, 10), (3000, 31, 6), (2000, 200, 16), (1500, 300, 4), (400, 160, 100)]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ------------------------------------------------------------------ the generator, restated
_U64 = np.uint64


def _smix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
    return x ^ (x >> _U64(31))


def _row_key(seed, stream, rows):
    with np.errstate(over="ignore"):
        base = _smix64(np.array([seed], dtype=np.uint64) ^ np.array([(stream * 0xD1342543DE82EF95) % 2**64], dtype=np.uint64))
        return _smix64(base + np.asarray(rows, dtype=np.uint64))


def _words(keys, n_words):
    p = np.arange(n_words, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return _smix64(keys[:, None] + p[None, :] * _U64(0xA0761D6478BD642F))


def _normals(seed, stream, rows, count):
    """(len(rows), count): normal 2p and 2p + 1 are the two Box-Muller branches of word p of the row's stream."""
    w = _words(_row_key(seed, stream, rows), max((count + 1) // 2, 1))
    u1 = ((w >> _U64(40)) + _U64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((w >> _U64(16)) & _U64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty((len(rows), 2 * w.shape[1]))
    out[:, 0::2], out[:, 1::2] = r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
    return out[:, :count]


def _choice_uniform(seed, rows):
    w = _words(_row_key(seed, 7, rows), 1)[:, 0]
    return ((w >> _U64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def _upper_factor(covs, x, sigma, c):
    """U with Sigma = U U^T, upper triangular: the reverse-order Cholesky factor of Sigma; where rounding makes Sigma
    indefinite (a model whose rows of C span 1e8), sigma L^-T of M = C_o^T C_o + sigma^2 I = L L^T -- the same factor
    up to rounding."""
    try:
        return np.linalg.cholesky(covs[:, ::-1, ::-1])[:, ::-1, ::-1]
    except np.linalg.LinAlgError:
        out = np.empty_like(covs)
        for i, cv in enumerate(covs):
            try:
                out[i] = np.linalg.cholesky(cv[::-1, ::-1])[::-1, ::-1]
            except np.linalg.LinAlgError:
                co = c[np.isfinite(x[i])]
                low = np.linalg.cholesky(co.T @ co + sigma ** 2 * np.eye(c.shape[1]))
                out[i] = sigma * np.linalg.inv(low).T
        return out


def _draw(x, sigma, c, mu, states, covs, seed, rows, keep_observed):
    """x_i = C (z_i + U_i eps_i) + mean + sigma eta_i, U_i the reverse-order Cholesky factor of Sigma_i."""
    d, k = c.shape
    out = mu + sigma * _normals(seed, 6, rows, d)
    if k > 0:
        u = _upper_factor(covs, x, sigma, c)
        z = states + np.einsum("nab,nb->na", u, _normals(seed, 5, rows, k))
        out = out + z @ c.T
    if keep_observed:
        out = np.where(np.isfinite(x), x, out)
    return out


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    kt = min(5, d)
    x = rng.standard_normal((n, kt)) @ rng.standard_normal((kt, d)) + 0.3 * rng.standard_normal((n, d)) + rng.standard_normal(d)
    x[rng.random((n, d)) < 0.3] = np.nan
    x[[3, n // 2]] = np.nan  # all-masked rows
    x[1, 2] = np.inf  # masked as everywhere else
    w = rng.uniform(0.5, 2.0, n)
    return x, w


def _model(rng, d, k):
    return 0.9, 0.5 * rng.standard_normal((d, k)), 0.3 * rng.standard_normal(d)


def _check_rows(got, want, x=None):
    scale = np.maximum(np.abs(want).max(axis=1), 1e-300)
    err = (np.abs(got - want).max(axis=1) / scale).max()
    assert err < TOL, err
    if x is not None:
        ob = np.isfinite(x)
        assert np.array_equal(got[ob], x[ob])  # bit-exact pass-through


# ------------------------------------------------------------------ 1. exact restatement
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_draws_match_the_restatement(P, oracle, n, d, k):
    rng = np.random.default_rng(n + d + k)
    x, w = _data(n, d, d + k)
    s, c, mu = _model(rng, d, k)
    xn = np.where(np.isfinite(x), x, np.nan)
    states, covs = oracle.infer(xn, s, c, mu)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    rows = np.arange(n)
    for keep in (False, True):
        out = m.sample_posterior(ds, seed=1234, keep_observed=keep)
        got = out.numpy()
        assert got.shape == (n, d) and np.all(np.isfinite(got))
        _check_rows(got, _draw(xn, s, c, mu, states, covs, 1234, rows, keep), xn if keep else None)
        assert np.array_equal(out.weights(), w)


# ------------------------------------------------------------------ 2. independence of where and how
_CHILD = ("import sys; sys.path.insert(0, %r); import numpy as np, ppca_rs_amd as P;"
          "g = np.load(sys.argv[1]); ds, m = P.Dataset(g['x'], g['w']), P.PPCAModel(float(g['s']), g['c'], g['mu']);"
          "np.save(sys.argv[2], np.stack([m.sample_posterior(ds, seed=99, keep_observed=b).numpy() for b in (False, True)]))")


@pytest.mark.parametrize("n,d,k", [(20000, 256, 10), (3000, 200, 16)])
def test_draws_do_not_depend_on_grid_path_or_split(P, n, d, k):
    import subprocess
    import sys
    import tempfile

    from ppca_rs_amd import _lib

    rng = np.random.default_rng(5 + k)
    x, w = _data(n, d, 40 + k)
    s, c, mu = _model(rng, d, k)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    base = np.stack([m.sample_posterior(ds, seed=99, keep_observed=b).numpy() for b in (False, True)])
    again = np.stack([m.sample_posterior(ds, seed=99, keep_observed=b).numpy() for b in (False, True)])
    assert np.array_equal(base, again)  # same seed: bit-identical
    other = m.sample_posterior(ds, seed=100).numpy()
    assert np.abs(other - base[0]).max() > 1e-3 * np.abs(base[0]).max()
    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(3)  # a few workgroups, hundreds of tiles each
        lim = np.stack([m.sample_posterior(ds, seed=99, keep_observed=b).numpy() for b in (False, True)])
    finally:
        ctx.set_grid_limit(0)
    assert _rel(lim, base) < 1e-9
    parts = list(ds.chunks(3))
    assert len(parts) == 3
    starts = np.cumsum([0] + [len(p) for p in parts])[:-1]
    cat = np.concatenate([m.sample_posterior(p, seed=99, row_offset=int(s0)).numpy() for p, s0 in zip(parts, starts)])
    assert _rel(cat, base[0]) < 1e-9
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        np.savez(os.path.join(td, "in.npz"), x=x, w=w, s=s, c=c, mu=mu)
        for env in ({"PPCA_RECON8": "0"}, {"PPCA_GEN_CHUNK": "256"}):
            out = os.path.join(td, "out.npy")
            subprocess.run([sys.executable, "-c", _CHILD % root, os.path.join(td, "in.npz"), out], check=True,
                           env={**os.environ, **env}, timeout=600)
            assert _rel(np.load(out), base) < 1e-9, env


def test_draws_do_not_depend_on_the_row_chunks(P, monkeypatch):
    """PPCA_POST_CHUNK=64 at n = 150: three chunks of the posterior scratch, the last of 22 rows, against one chunk -- bit for bit,
    in both modes, under a row offset and for a mixture (components of k = 2 and k = 3, each drawing the rows that chose it)."""
    n, d, k = 150, 13, 3
    rng = np.random.default_rng(71)
    x, w = _data(n, d, 72)
    s, c, mu = _model(rng, d, k)
    ds = P.Dataset(x, w)
    m = P.PPCAModel(s, c, mu)
    mix = P.PPCAMix([P.PPCAModel(0.8, 0.5 * rng.standard_normal((d, 2)), 0.3 * rng.standard_normal(d)), m], np.log([0.4, 0.6]))

    def draws():
        return {(name, keep, off): model.sample_posterior(ds, seed=99, keep_observed=keep, row_offset=off).numpy()
                for name, model in (("model", m), ("mixture", mix)) for keep in (False, True) for off in (0, 1000)}

    base = draws()
    monkeypatch.setenv("PPCA_POST_CHUNK", "64")
    chunked = draws()
    monkeypatch.delenv("PPCA_POST_CHUNK")
    assert not np.array_equal(base["model", False, 0], base["model", False, 1000])  # (the offset reaches the keys)
    for case, a in chunked.items():
        assert np.array_equal(a, base[case]), (case, np.argwhere(a != base[case])[:8])


# ------------------------------------------------------------------ 3. the Gram guard's fallback
def test_draws_of_a_guard_tripping_model(P, oracle):
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
    states, covs = oracle.infer(xn, s, c, mu)
    for keep in (False, True):
        got = m.sample_posterior(ds, seed=7, keep_observed=keep).numpy()
        assert np.all(np.isfinite(got))
        want = _draw(xn, s, c, mu, states, covs, 7, np.arange(n), keep)
        # where dimension 0 is observed, Sigma's eigenvalues span ~1e16 and the fp64 factor of its small directions is
        # rounding on either side: those rows are held to finiteness (and impute's pass-through) only
        sel = ~np.isfinite(xn[:, 0])
        assert sel.sum() > 200
        _check_rows(got[sel][:, 1:], want[sel][:, 1:], xn[sel][:, 1:] if keep else None)
        assert _rel(got[sel][:, 0], want[sel][:, 0]) < TOL  # C_0 w cancels: held to the column's scale
        if keep:
            ob = np.isfinite(xn)
            assert np.array_equal(got[ob], xn[ob])


# ------------------------------------------------------------------ 4. distribution
def test_draws_have_the_posterior_predictive_distribution(P):
    rng = np.random.default_rng(21)
    d, k, n = 64, 6, 200_000
    s, c, mu = 0.7, 0.8 * rng.standard_normal((d, k)), rng.standard_normal(d)
    row = c @ rng.standard_normal(k) + mu + s * rng.standard_normal(d)
    row[rng.random(d) < 0.4] = np.nan
    m = P.PPCAModel(s, c, mu)
    one = P.Dataset(row[None, :])
    inf = m.infer(one)
    mean = m.smooth(one).numpy()[0]
    cov = inf.smoothed_covariances(m)[0]
    var = inf.smoothed_covariances_diagonal(m).numpy()[0]
    assert _rel(np.diag(cov), var) < 1e-10
    draws = m.sample_posterior(P.Dataset(np.tile(row, (n, 1))), seed=2024).numpy()
    got_mean = draws.mean(axis=0)
    assert np.all(np.abs(got_mean - mean) < 5 * np.sqrt(var / n))
    got_var = draws.var(axis=0, ddof=1)
    assert np.all(np.abs(got_var / var - 1) < 0.02)
    blk = slice(0, 12)
    dc = draws[:, blk] - got_mean[blk]
    got_cov = dc.T @ dc / (n - 1)
    want = cov[blk, blk]
    se = np.sqrt((np.outer(var[blk], var[blk]) + want ** 2) / n)
    assert np.all(np.abs(got_cov - want) < 5 * se)
    # impute: observed entries fixed, masked ones with the extrapolated variances
    imp = m.sample_posterior(P.Dataset(np.tile(row, (n, 1))), seed=2025, keep_observed=True).numpy()
    ob = np.isfinite(row)
    assert np.all(imp[:, ob] == row[ob])
    evar = inf.extrapolated_covariances_diagonal(m, one).numpy()[0]
    assert np.all(evar[ob] == 0.0)
    assert np.all(np.abs(imp[:, ~ob].var(axis=0, ddof=1) / evar[~ob] - 1) < 0.02)


# ------------------------------------------------------------------ 5. mixture
def _mix_case(oracle, rng):
    d, k, nm, n = 20, 3, 3, 600
    x = np.concatenate([oracle.synth(n // nm, d, k, 0.3, 500 + c_, mean_scale=2.0)[0] for c_ in range(nm)])
    x[7] = np.nan
    return x, rng.uniform(0.5, 2.0, x.shape[0])


@pytest.mark.parametrize("ks", [(3, 3, 3), (4, 20)])
def test_mixture_draws(P, oracle, ks):
    rng = np.random.default_rng(19)
    x, w = _mix_case(oracle, rng)
    n, d = x.shape
    nm = len(ks)
    sig = np.array([0.8, 1.1, 0.6])[:nm]
    cs = [rng.standard_normal((d, k)) for k in ks]
    ms = rng.standard_normal((nm, d))
    lw = np.log(np.array([0.5, 0.2, 0.3])[:nm] / np.array([0.5, 0.2, 0.3])[:nm].sum())
    ds = P.Dataset(x, w)
    mix = P.PPCAMix([P.PPCAModel(sig[c_], cs[c_], ms[c_]) for c_ in range(nm)], lw)
    post = np.exp(mix.infer_cluster(ds))
    seed, rows = 31, np.arange(n)
    u = _choice_uniform(seed, rows)
    cum = np.cumsum(post, axis=1)
    pick = np.minimum((u[:, None] >= cum).sum(axis=1), nm - 1)
    clear = np.abs(u[:, None] - cum).min(axis=1) > 1e-9
    assert clear.mean() > 0.99
    xn = np.where(np.isfinite(x), x, np.nan)
    for keep in (False, True):
        out = mix.sample_posterior(ds, seed=seed, keep_observed=keep)
        got = out.numpy()
        assert np.all(out.weights() == 1.0)  # the mixture's outputs carry no weights
        want = np.empty_like(got)
        for c_ in range(nm):
            st, cv = oracle.infer(xn, sig[c_], cs[c_], ms[c_])
            want[pick == c_] = _draw(xn, sig[c_], cs[c_], ms[c_], st, cv, seed, rows, keep)[pick == c_]
        _check_rows(got[clear], want[clear], xn[clear] if keep else None)
    # component frequencies over replicated rows: a row whose posterior is spread over the components
    i = int(np.argmax(np.sort(post, axis=1)[:, -2]))
    N = 200_000
    big = P.Dataset(np.tile(x[i], (N, 1)))
    draws = mix.sample_posterior(big, seed=8).numpy()
    # the component the device chose for each copy: the one whose restated draw the copy is
    xi = np.tile(xn[i], (N, 1))
    cand = []
    for c_ in range(nm):
        st, cv = oracle.infer(xn[i][None, :], sig[c_], cs[c_], ms[c_])
        cand.append(_draw(xi, sig[c_], cs[c_], ms[c_], np.repeat(st, N, 0), np.repeat(cv, N, 0), 8, np.arange(N), False))
    dist = np.stack([np.abs(draws - w_).max(axis=1) / np.abs(w_).max(axis=1) for w_ in cand], axis=1)
    chosen = dist.argmin(axis=1)
    assert np.all(dist[np.arange(N), chosen] < TOL)
    freq = np.bincount(chosen, minlength=nm) / N
    assert np.all(np.abs(freq - post[i]) < 5 * np.sqrt(post[i] * (1 - post[i]) / N) + 1e-12), (freq, post[i])


# ------------------------------------------------------------------ 6. edges
def test_edges(P):
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(4)
    d = 12
    s, c, mu = 0.5, rng.standard_normal((d, 3)), rng.standard_normal(d)
    m = P.PPCAModel(s, c, mu)
    empty = P.Dataset(np.zeros((0, d)))
    assert len(m.sample_posterior(empty, seed=1)) == 0
    mix = P.PPCAMix([m, P.PPCAModel(0.7, c, mu)], np.log([0.5, 0.5]))
    assert len(mix.sample_posterior(empty, seed=1)) == 0
    # state size 0: x = mean + sigma eta (observed entries kept by impute)
    x = rng.standard_normal((50, d))
    x[rng.random((50, d)) < 0.3] = np.nan
    m0 = P.PPCAModel(s, np.zeros((d, 0)), mu)
    want = mu + s * _normals(3, 6, np.arange(50), d)
    _check_rows(m0.sample_posterior(P.Dataset(x), seed=3).numpy(), want)
    _check_rows(m0.sample_posterior(P.Dataset(x), seed=3, keep_observed=True).numpy(), np.where(np.isfinite(x), x, want), x)
    # bad arguments
    ds = P.Dataset(x)
    h = C.c_void_p()
    dev = m._device(ds._ctx).h
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_posterior_sample(ds._ctx.handle, ds._h, dev, 2, 1, 0, C.byref(h)))
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_posterior_sample(ds._ctx.handle, ds._h, dev, 0, 1, 0, None))
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_posterior_sample(ds._ctx.handle, ds._h, dev, 0, 1, -1, C.byref(h)))
    devs, arr = mix._handles(ds._ctx)
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_mix_posterior_sample(ds._ctx.handle, ds._h, arr, _lib.ptr(mix._lw), 2, 5, 1, 0, C.byref(h)))
    with pytest.raises(P.PPCAError):
        _lib.check(_lib.lib().ppca_mix_posterior_sample(ds._ctx.handle, ds._h, arr, _lib.ptr(mix._lw), 2, 0, 1, 0, None))
    with pytest.raises(P.PPCAError):
        m.sample_posterior(P.Dataset(np.zeros((3, d + 1))), seed=1)
    with pytest.raises(ValueError):
        m.sample_posterior(ds, seed=1, row_offset=-1)
    assert m.sample_posterior(ds).numpy().shape == (50, d)  # seed=None: a fresh seed
