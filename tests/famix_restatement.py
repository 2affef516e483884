"""Dense numpy restatement of the mixture of factor analysers with shared column noise (x | c = C_c z + mean_c + eps, eps_j ~ N(0, psi_j^2),
P(c) = pi_c), shared by tests/test_famix_host.py and tests/test_gpu_factor_mixture.py.  Everything works in the ORIGINAL units of the
columns: no whitening, no packed buffers, nothing of the library.  Masked entries are the non-finite ones.

`llks` / `log_posteriors` use the dense m x m Gaussian of every row and component (fa_restatement.llks).  `iterate` and `smooth` take
the same densities from the k x k form of the same Gaussian (`estep`: the determinant lemma and the Woodbury identity, batched over the
rows) so that a restated step takes a second, not a minute; tests/test_famix_host.py holds the two forms together."""
import numpy as np

import fa_restatement as F

LN_2PI = F.LN_2PI


def _logsumexp(a, axis):
    mx = a.max(axis=axis, keepdims=True)
    return (mx + np.log(np.exp(a - mx).sum(axis=axis, keepdims=True))).squeeze(axis)


def log_softmax(v):
    v = np.asarray(v, dtype=np.float64)
    return v - _logsumexp(v, 0)


def component_llks(x, psi, cs, mus):
    """(K, N): the dense log-density of every row under every component."""
    return np.stack([F.llks(x, psi, c, mu) for c, mu in zip(cs, mus)])


def llks(x, psi, cs, mus, logw):
    """Per-row log-density of the mixture; 0 for a row with no observed entry."""
    return _logsumexp(component_llks(x, psi, cs, mus) + log_softmax(logw)[:, None], 0)


def log_posteriors(x, psi, cs, mus, logw):
    """(N, K) log P(c | x_i); the prior weights for a row with no observed entry."""
    u = component_llks(x, psi, cs, mus) + log_softmax(logw)[:, None]
    return (u - _logsumexp(u, 0)).T


def estep(x, psi, c, mu):
    """One component, all rows at once: z (N, k), Sigma (N, k, k) and the row's log-density from Sigma = (I + C_O^T Psi_O^-1 C_O)^-1,
    z = Sigma C_O^T Psi_O^-1 r: ln N = -1/2 (r^T Psi^-1 r - z^T Sigma^-1 z + sum ln psi_O^2 - ln det Sigma + m ln 2 pi)."""
    n, d = x.shape
    k = c.shape[1]
    obs = np.isfinite(x)
    r = np.where(obs, x - mu, 0.0)
    ip = 1.0 / psi ** 2
    gram = (obs.astype(np.float64) @ (ip[:, None, None] * c[:, :, None] * c[:, None, :]).reshape(d, k * k)).reshape(n, k, k) + np.eye(k)
    sigma = np.linalg.inv(gram)
    b = (r * ip) @ c
    z = np.einsum("nab,nb->na", sigma, b)
    quad = (r * r * ip).sum(1) - (b * z).sum(1)
    logdet = obs @ np.log(psi ** 2) + np.linalg.slogdet(gram)[1]
    ll = np.where(obs.any(1), -0.5 * (quad + logdet + obs.sum(1) * LN_2PI), 0.0)
    return z, sigma, ll


def responsibilities(x, psi, cs, mus, logw):
    """([estep of every component], r (N, K), the rows' mixture log-densities) from the k x k form."""
    es = [estep(x, psi, c, mu) for c, mu in zip(cs, mus)]
    u = np.stack([e[2] for e in es]) + log_softmax(logw)[:, None]
    lse = _logsumexp(u, 0)
    return es, np.exp(u - lse).T, lse


def moments(x, wr, z, sigma, mu):
    """The E-step sums of one component in original units (fa_restatement.moments, all rows at once) under the row weights wr."""
    n, d = x.shape
    k = z.shape[1]
    obs = np.isfinite(x)
    wm = wr[:, None] * obs
    r = np.where(obs, x - mu, 0.0)
    P = z[:, :, None] * z[:, None, :] + sigma
    return (wm * r).T @ z, (wm.T @ P.reshape(n, k * k)).reshape(d, k, k), wm.T @ z, (wm * r).sum(0), wm.sum(0), (wm * r * r).sum(0)


def mstep(moms, psi, cs, mus, min_noise=None):
    """The M-step from the components' moments (moms[c] = cross, S, U, sumx, tot, sq of `moments`): per component and column the
    transform row, then the mean given the new row (fa_restatement.iterate; a column whose S_cj is not positive definite keeps its row);
    then ONE noise level per column from the residual sums of all components pooled."""
    d = psi.shape[0]
    num, den = np.zeros(d), np.zeros(d)
    cs1, mus1 = [], []
    for (cross, S, U, sumx, tot, sq), c, mu in zip(moms, cs, mus):
        c1, mu1 = c.copy(), mu.copy()
        for j in range(d):
            try:
                np.linalg.cholesky(S[j])
                c1[j] = np.linalg.solve(S[j], cross[j])
            except np.linalg.LinAlgError:
                pass
            if tot[j] > 0.0:
                delta = (sumx[j] - c1[j] @ U[j]) / tot[j]
                mu1[j] = mu[j] + delta
                num[j] += sq[j] - 2.0 * c1[j] @ cross[j] + c1[j] @ S[j] @ c1[j] - delta * delta * tot[j]
                den[j] += tot[j]
        cs1.append(c1)
        mus1.append(mu1)
    psi1 = psi.copy()
    for j in range(d):
        if den[j] > 0.0:
            v = num[j] / den[j]
            if np.isfinite(v) and v > 0.0:
                psi1[j] = np.sqrt(v)
        if min_noise is not None:
            psi1[j] = max(psi1[j], min_noise[j])
    return psi1, cs1, mus1


def iterate(x, w, psi, cs, mus, logw, min_noise=None):
    """One ECM iteration.  Responsibilities from the input model; row weights w_i r_ic (rows with w_i <= 0 contribute nothing); `mstep`;
    new log-weights log_softmax(ln sum_i w_i r_ic).
    Returns (psi, [C_c], [mean_c], log-weights, llk of the INPUT model = sum_i w_i llks_i)."""
    es, resp, lse = responsibilities(x, psi, cs, mus, logw)
    wpos = np.where(w > 0.0, w, 0.0)
    moms = [moments(x, wpos * resp[:, q], es[q][0], es[q][1], mu) for q, mu in enumerate(mus)]
    psi1, cs1, mus1 = mstep(moms, psi, cs, mus, min_noise)
    with np.errstate(divide="ignore"):
        lw1 = log_softmax(np.log((wpos[:, None] * resp).sum(0)))
    return psi1, cs1, mus1, lw1, float(w @ lse)


def smooth(x, psi, cs, mus, logw):
    """sum_c r_ic (C_c z_ic + mean_c) for every entry."""
    es, resp, _ = responsibilities(x, psi, cs, mus, logw)
    return sum(resp[:, q, None] * (es[q][0] @ c.T + mu) for q, (c, mu) in enumerate(zip(cs, mus)))


def synth(n, d, k, n_models, psi, mask, seed, separation=1.0, signal=3.0, own=1.0):
    """Rows from a random mixture with the given noise levels, components equally likely: component c is fa_restatement.synth's model
    with mean_c = psi (offset + separation * e_c), offset and e_c standard normal per column -- the component means are separated by
    about separation * sqrt(2) noise levels in every column's own units, whatever the column's scale.  The loadings of component c are
    common + own * e_c before they are scaled: own < 1 gives components that share most of their subspace, so that with a small
    separation many rows keep weight in several components.
    Returns (x, [C_c], [mean_c], the rows' components)."""
    rng = np.random.default_rng(seed)
    offset, common, size = rng.standard_normal(d), rng.standard_normal((d, k)), rng.uniform(0.3, 1.0, (d, 1))
    cs, mus = [], []
    for _ in range(n_models):
        load = common + own * rng.standard_normal((d, k)) if own < 1.0 else rng.standard_normal((d, k))
        load *= signal * (size if own < 1.0 else rng.uniform(0.3, 1.0, (d, 1))) / np.linalg.norm(load, axis=1, keepdims=True)
        cs.append(load * psi[:, None])
        mus.append(psi * (offset + separation * rng.standard_normal(d)))
    which = rng.integers(0, n_models, n)
    x = np.empty((n, d))
    for q in range(n_models):
        idx = np.nonzero(which == q)[0]
        x[idx] = rng.standard_normal((idx.size, k)) @ cs[q].T + mus[q] + psi * rng.standard_normal((idx.size, d))
    x[rng.random((n, d)) < mask] = np.nan
    return x, cs, mus, which
