"""Dense numpy restatement of masked factor analysis (x = C z + mean + eps, eps_j ~ N(0, psi_j^2)), shared by tests/test_fa_host.py and
tests/test_gpu_factor_noise.py.  Everything here works row by row in the ORIGINAL units of the columns: no whitening, no packed
buffers, nothing of the library.  Masked entries are the non-finite ones."""
import numpy as np

LN_2PI = float(np.log(2.0 * np.pi))


def llks(x, psi, c, mu):
    """Per-row log-density under N(mu_O, C_O C_O^T + diag(psi_O^2)); 0 for a row with no observed entry."""
    out = np.zeros(x.shape[0])
    for i, row in enumerate(x):
        o = np.isfinite(row)
        m = int(o.sum())
        if m == 0:
            continue
        cov = c[o] @ c[o].T + np.diag(psi[o] ** 2)
        r = row[o] - mu[o]
        sign, logdet = np.linalg.slogdet(cov)
        out[i] = -0.5 * (r @ np.linalg.solve(cov, r) + logdet + m * LN_2PI)
    return out


def posterior(row, psi, c, mu):
    """(z, Sigma) of one row: Sigma = (I + C_O^T Psi_O^-1 C_O)^-1, z = Sigma C_O^T Psi_O^-1 (x_O - mu_O)."""
    o = np.isfinite(row)
    k = c.shape[1]
    co = c[o] / psi[o, None] ** 2
    sigma = np.linalg.inv(np.eye(k) + co.T @ c[o])
    return sigma @ (co.T @ (row[o] - mu[o])), sigma


def moments(x, w, psi, c, mu):
    """The E-step sums in original units, per column j over its observed rows: cross_j = sum w (x_j - mu_j) z, S_j = sum w (z z^T + Sigma),
    U_j = sum w z, sumx_j = sum w (x_j - mu_j), tot_j = sum w, sq_j = sum w (x_j - mu_j)^2."""
    n, d = x.shape
    k = c.shape[1]
    cross, S, U = np.zeros((d, k)), np.zeros((d, k, k)), np.zeros((d, k))
    sumx, tot, sq = np.zeros(d), np.zeros(d), np.zeros(d)
    for i in range(n):
        o = np.isfinite(x[i])
        if not o.any():
            continue
        z, sigma = posterior(x[i], psi, c, mu)
        r = x[i, o] - mu[o]
        cross[o] += w[i] * np.outer(r, z)
        S[o] += w[i] * (np.outer(z, z) + sigma)
        U[o] += w[i] * z
        sumx[o] += w[i] * r
        tot[o] += w[i]
        sq[o] += w[i] * r * r
    return cross, S, U, sumx, tot, sq


def iterate(x, w, psi, c, mu, min_noise=None):
    """One ECM iteration: per column the transform row given the old mean and noise, then the mean given the new row, then the noise
    given both.  A column whose S_j is not positive definite keeps its row; one with no observed entry keeps everything."""
    cross, S, U, sumx, tot, sq = moments(x, w, psi, c, mu)
    d = x.shape[1]
    psi1, c1, mu1 = psi.copy(), c.copy(), mu.copy()
    for j in range(d):
        try:
            np.linalg.cholesky(S[j])
            c1[j] = np.linalg.solve(S[j], cross[j])
        except np.linalg.LinAlgError:
            pass
        if tot[j] > 0.0:
            delta = (sumx[j] - c1[j] @ U[j]) / tot[j]
            mu1[j] = mu[j] + delta
            v = (sq[j] - 2.0 * c1[j] @ cross[j] + c1[j] @ S[j] @ c1[j] - delta * delta * tot[j]) / tot[j]
            if np.isfinite(v) and v > 0.0:
                psi1[j] = np.sqrt(v)
        if min_noise is not None:
            psi1[j] = max(psi1[j], min_noise[j])
    return psi1, c1, mu1


def synth(n, d, k, psi, mask, seed, signal=3.0):
    """Rows drawn from a random FA model with the given noise levels: x_j = psi_j (signal-scaled loadings . z + offset + eps_j), so that
    the signal variance of column j is at most signal^2 psi_j^2; entries masked with probability `mask`.  Returns (x, c, mu)."""
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((d, k))
    load *= signal * rng.uniform(0.3, 1.0, (d, 1)) / np.linalg.norm(load, axis=1, keepdims=True)
    c = load * psi[:, None]
    mu = psi * rng.standard_normal(d)
    x = rng.standard_normal((n, k)) @ c.T + mu + psi * rng.standard_normal((n, d))
    x[rng.random((n, d)) < mask] = np.nan
    return x, c, mu
