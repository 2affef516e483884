"""Student-t PPCA for masked data, restated row by row in numpy (nothing of the library): the model of DESIGN.md section 4.15 in its
DIRECT form -- the rows' weights u inside the sums, no scaled dataset.

For a row with observed set O (m entries), x~ = x_O - mean_O and the model (sigma, C, mean, nu):
    delta = x~^T (C_O C_O^T + sigma^2 I)^-1 x~          the dense m x m solve (d <= 64 by default; the k x k form beyond)
    u     = (nu + m) / (nu + delta)
    ell   = ln Gamma((nu + m) / 2) - ln Gamma(nu / 2) - (m / 2) ln(nu pi) - 1/2 ln det(C_O C_O^T + sigma^2 I)
            - 1/2 (nu + m) log1p(delta / nu)
A row without an observed entry has delta = 0, u = 1, ell = 0."""
import math

import numpy as np


def digamma(x):
    """psi(x), x > 0: upward recurrence to x >= 10, then the asymptotic series."""
    s = 0.0
    while x < 10.0:
        s -= 1.0 / x
        x += 1.0
    r2 = 1.0 / (x * x)
    return s + math.log(x) - 0.5 / x - r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 / 132))))


def tables(d, nu):
    """lg[m], g[m] for m = 0 .. d"""
    lg = np.array([math.lgamma(0.5 * (nu + m)) - math.lgamma(0.5 * nu) - 0.5 * m * math.log(nu * math.pi) for m in range(d + 1)])
    g = np.array([digamma(0.5 * (nu + m)) - math.log(0.5 * (nu + m)) for m in range(d + 1)])
    return lg, g


def estep(x, w, sigma, c, mu, nu, dense=None):
    """The per-row quantities and the statistics of one E-step.  dense: delta and ln det by the m x m covariance (default: d <= 64),
    otherwise by the k x k forms delta = (|r|^2 + sigma^2 |z|^2) / sigma^2, ln det = (m - k) ln sigma^2 + ln det M."""
    n, d = x.shape
    k = c.shape[1]
    dense = d <= 64 if dense is None else dense
    w = np.ones(n) if w is None else w
    s2 = sigma * sigma
    r = dict(delta=np.zeros(n), u=np.ones(n), ell=np.zeros(n), m=np.zeros(n, dtype=np.int64), z=np.zeros((n, k)),
             cross=np.zeros((d, k)), S=np.zeros((d, k, k)), totals=np.zeros(d), V=np.zeros((d, k)), A=np.zeros(d), T=np.zeros(d),
             sq=np.zeros(d))
    # what each sum is a sum OF (the measure of its rounding)
    r["abs"] = dict(V=np.zeros((d, k)), A=np.zeros(d), T=np.zeros(d), sq=np.zeros(d))
    q_terms = np.zeros(n)
    g = tables(d, nu)[1]
    for i in range(n):
        o = np.isfinite(x[i])
        m = int(o.sum())
        r["m"][i] = m
        q_terms[i] = g[0] - 1.0
        if m == 0:
            continue
        co, xt = c[o], x[i, o] - mu[o]
        M = s2 * np.eye(k) + co.T @ co
        z = np.linalg.solve(M, co.T @ xt)
        Sig = s2 * np.linalg.inv(M)
        if dense:
            cov = co @ co.T + s2 * np.eye(m)
            delta = float(xt @ np.linalg.solve(cov, xt))
            logdet = np.linalg.slogdet(cov)[1]
        else:
            res = xt - co @ z
            delta = float(res @ res + s2 * (z @ z)) / s2
            logdet = (m - k) * math.log(s2) + np.linalg.slogdet(M)[1]
        u = (nu + m) / (nu + delta)
        ell = (math.lgamma(0.5 * (nu + m)) - math.lgamma(0.5 * nu) - 0.5 * m * math.log(nu * math.pi) - 0.5 * logdet
               - 0.5 * (nu + m) * math.log1p(delta / nu))
        r["delta"][i], r["u"][i], r["ell"][i], r["z"][i] = delta, u, ell, z
        q_terms[i] = g[m] + math.log(u) - u
        wi, wu = w[i], w[i] * u
        r["cross"][o] += wu * np.outer(xt, z)
        r["S"][o] += wi * (Sig + u * np.outer(z, z))
        r["totals"][o] += wi
        r["V"][o] += wu * z
        r["A"][o] += wu * xt
        r["T"][o] += wu
        r["sq"][o] += wu * xt * xt
        r["abs"]["V"][o] += abs(wu) * np.abs(z)
        r["abs"]["A"][o] += abs(wu) * np.abs(xt)
        r["abs"]["T"][o] += abs(wu)
        r["abs"]["sq"][o] += abs(wu) * xt * xt
    r["scalars"] = np.array([w.sum(), (w * r["ell"]).sum(), (w * q_terms).sum(), float((r["m"] > 0).sum())])
    r["scalars_abs"] = np.array([np.abs(w).sum(), (np.abs(w) * np.abs(r["ell"])).sum(), (np.abs(w) * np.abs(q_terms)).sum(), 1.0])
    return r


def llks(x, sigma, c, mu, nu, dense=None):
    return estep(x, None, sigma, c, mu, nu, dense)["ell"]


def dof_root(q, lo=0.5, hi=1e4):
    """The root of ln(nu / 2) - psi(nu / 2) + 1 + q = 0 by bisection on [lo, hi]; the upper end when there is no sign change."""
    def f(nu):
        return math.log(0.5 * nu) - digamma(0.5 * nu) + 1.0 + q
    if not (f(lo) > 0.0 and f(hi) < 0.0):
        return hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-13 * hi:
            break
    return 0.5 * (lo + hi)


def mstep(sigma, c, mu, e):
    """Steps 1-3 from the statistics of estep: (sigma, C, mean)."""
    d, k = c.shape
    c1, mu1 = c.copy(), mu.copy()
    num = 0.0
    for j in range(d):
        try:
            np.linalg.cholesky(e["S"][j])
            c1[j] = np.linalg.solve(e["S"][j], e["cross"][j])
        except np.linalg.LinAlgError:  # a pivot <= 0 keeps the old row
            pass
        delta = (e["A"][j] - c1[j] @ e["V"][j]) / e["T"][j] if e["T"][j] > 0 else 0.0
        mu1[j] += delta
        num += e["sq"][j] - 2.0 * c1[j] @ e["cross"][j] + c1[j] @ e["S"][j] @ c1[j] - delta * delta * e["T"][j]
    v = num / e["totals"].sum()
    return (math.sqrt(v) if np.isfinite(v) and v > 0 else sigma), c1, mu1


def iterate(x, w, sigma, c, mu, nu, estimate_dof=False, dense=None):
    """One ECM step: ((sigma, C, mean, nu) of the next model, t log-likelihood of THIS model)."""
    e = estep(x, w, sigma, c, mu, nu, dense)
    s1, c1, mu1 = mstep(sigma, c, mu, e)
    nu1 = dof_root(e["scalars"][2] / e["scalars"][0]) if estimate_dof else nu
    return (s1, c1, mu1, nu1), e["scalars"][1]


def synth_contaminated(n, d, k, frac, seed, noise=0.5, mask=0.3, spread=12.0):
    """(x, C_true, mean_true, bad): rows C z + mean + noise eps with `mask` of the entries masked; a share `frac` of the rows (bad) is
    replaced by mean + spread N(0, I) before masking."""
    rng = np.random.default_rng(seed)
    c, mu = rng.standard_normal((d, k)), rng.standard_normal(d)
    x = rng.standard_normal((n, k)) @ c.T + mu + noise * rng.standard_normal((n, d))
    bad = np.zeros(n, dtype=bool)
    bad[rng.permutation(n)[:int(round(frac * n))]] = True
    x[bad] = mu + spread * rng.standard_normal((int(bad.sum()), d))
    x[rng.random((n, d)) < mask] = np.nan
    return x, c, mu, bad


def subspace_angle(a, b):
    """The largest principal angle between the column spaces of a and b, in degrees."""
    qa, qb = np.linalg.qr(a)[0], np.linalg.qr(b)[0]
    s = np.linalg.svd(qa.T @ qb, compute_uv=False)
    return float(np.degrees(np.arccos(np.clip(s.min(), -1.0, 1.0))))


def masked_case(n, d, k, seed):
    """(x, w, (sigma, C, mean)): 30 % masked, weights in [0.5, 2] with a few exact zeros (n >= 20), one all-masked row (n >= 3), one
    all-masked column (d >= 3); the model is near the one the rows were drawn from, not at it."""
    rng = np.random.default_rng(seed)
    c_true = rng.standard_normal((d, k))
    x = rng.standard_normal((n, k)) @ c_true.T + 0.5 * rng.standard_normal((n, d)) + rng.standard_normal(d)
    x[rng.random(x.shape) < 0.3] = np.nan
    if n >= 3:
        x[n // 2] = np.nan
    if d >= 3:
        x[:, d // 3] = np.nan
    w = rng.uniform(0.5, 2.0, n)
    if n >= 20:
        w[rng.permutation(n)[:max(1, n // 50)]] = 0.0
    return x, w, (0.8, 0.7 * c_true + 0.3 * rng.standard_normal((d, k)), 0.3 * rng.standard_normal(d))


# The contaminated case of the tests: N = 600, d = 12, k = 3, 30 % masked, 5 % of the rows replaced by mean + 12 N(0, I), true noise 0.5.
# With these seeds the restatement ends 2.25 degrees from the true subspace at nu = 4 and 73.9 degrees at nu = 1e12 after 30 steps.
CONTAMINATED = dict(n=600, d=12, k=3, frac=0.05, seed=2, start_seed=102)


def contaminated_start():
    """(x, C_true, contaminated rows, the random start's transform); the start is (sigma = 1, that transform, mean = 0)."""
    p = CONTAMINATED
    x, c, _, bad = synth_contaminated(p["n"], p["d"], p["k"], p["frac"], p["seed"])
    return x, c, bad, np.random.default_rng(p["start_seed"]).standard_normal(c.shape)
