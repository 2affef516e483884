"""PPCA with a known precision per entry, restated row by row in numpy (nothing of the library): the model of DESIGN.md section 4.16.

    x_ij = mean_j + c_j . z_i + eps_ij,   z_i ~ N(0, I_k),   eps_ij ~ N(0, sigma^2 / p_ij)

Entry (i, j) is observed iff x_ij is finite and p_ij is finite and > 0.  For a row with observed set O (m entries), x~ = x_O - mean_O:
    dense form (default for d <= 64)   cov = C_O C_O^T + sigma^2 diag(1 / p_O)                                         (m x m)
        ell = -1/2 [ x~^T cov^-1 x~ + ln det cov + m ln 2 pi ],   z = C_O^T cov^-1 x~,   Sigma = I - C_O^T cov^-1 C_O
    k x k form                         G = C_O^T diag(p_O) C_O, b = C_O^T diag(p_O) x~, M = sigma^2 I + G
        z = M^-1 b, Sigma = sigma^2 M^-1,
        ell = -1/2 [ (sum p x~^2 - b^T M^-1 b) / sigma^2 + ln det M + (m - k) ln sigma^2 + m ln 2 pi - sum ln p ]
A row with m = 0 has ell = 0, z = 0 (and Sigma = I).  Every sum of the statistics comes with the sum of its terms' magnitudes."""
import math

import numpy as np

LN_2PI = math.log(2.0 * math.pi)


def observed(x, p):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & np.isfinite(p) & (p > 0)


def row(xi, pi, sigma, c, mu, dense):
    """(ell, z, Sigma, m) of one row."""
    k = c.shape[1]
    o = observed(xi, pi)
    m = int(o.sum())
    if m == 0:
        return 0.0, np.zeros(k), np.eye(k), 0
    s2 = sigma * sigma
    co, xt, po = c[o], xi[o] - mu[o], pi[o]
    if dense:
        cov = co @ co.T + s2 * np.diag(1.0 / po)
        sol = np.linalg.solve(cov, np.column_stack([xt, co]))
        ell = -0.5 * (float(xt @ sol[:, 0]) + np.linalg.slogdet(cov)[1] + m * LN_2PI)
        z = co.T @ sol[:, 0]
        sig = np.eye(k) - co.T @ sol[:, 1:]
    else:
        M = s2 * np.eye(k) + (co * po[:, None]).T @ co
        b = co.T @ (po * xt)
        z = np.linalg.solve(M, b)
        sig = s2 * np.linalg.inv(M)
        ell = -0.5 * ((float((po * xt) @ xt) - float(b @ z)) / s2 + np.linalg.slogdet(M)[1] + (m - k) * math.log(s2) + m * LN_2PI
                      - float(np.log(po).sum()))
    return ell, z, 0.5 * (sig + sig.T), m


def estep(x, p, w, sigma, c, mu, dense=None):
    """The per-row quantities and the statistics of one E-step; r["abs"][name]: the sums of the terms' magnitudes."""
    n, d = x.shape
    k = c.shape[1]
    dense = d <= 64 if dense is None else dense
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    names = dict(cross=(d, k), S=(d, k, k), V=(d, k), A=(d,), T=(d,), sq=(d,), cnt=(d,))
    r = dict(ell=np.zeros(n), z=np.zeros((n, k)), Sigma=np.zeros((n, k, k)), m=np.zeros(n, dtype=np.int64))
    r.update({key: np.zeros(shape) for key, shape in names.items()})
    r["abs"] = {key: np.zeros(shape) for key, shape in names.items()}
    for i in range(n):
        ell, z, sig, m = row(x[i], p[i], sigma, c, mu, dense)
        r["ell"][i], r["z"][i], r["Sigma"][i], r["m"][i] = ell, z, sig, m
        if m == 0:
            continue
        o = observed(x[i], p[i])
        xt, wp = x[i, o] - mu[o], w[i] * p[i, o]
        P2 = sig + np.outer(z, z)
        terms = dict(cross=wp[:, None] * np.outer(xt, z), S=wp[:, None, None] * P2[None], V=wp[:, None] * z[None], A=wp * xt, T=wp,
                     sq=wp * xt * xt, cnt=np.full(m, w[i]))
        for key, t in terms.items():
            r[key][o] += t
            r["abs"][key][o] += np.abs(t)
    r["scalars"] = np.array([w.sum(), (w * r["ell"]).sum(), float((r["m"] > 0).sum())])
    r["scalars_abs"] = np.array([np.abs(w).sum(), (np.abs(w) * np.abs(r["ell"])).sum(), 1.0])
    return r


def tril(S):
    """(d, k, k) symmetric -> (d, k (k + 1) / 2) lower-packed, entry (a, b), a >= b, at a (a + 1) / 2 + b."""
    k = S.shape[-1]
    return np.stack([S[..., a, b] for a in range(k) for b in range(a + 1)], axis=-1)


def packed_stats(e, key=None):
    """cross | S packed | V | A | T | sq | cnt as the library lays them out (of e, or of e[key], e.g. "abs")."""
    s = e if key is None else e[key]
    return np.concatenate([s["cross"].ravel(), tril(s["S"]).ravel(), s["V"].ravel(), s["A"], s["T"], s["sq"], s["cnt"]])


def mstep(sigma, c, mu, e):
    """The ECM step from the statistics of estep: (sigma, C, mean)."""
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
    den = e["cnt"].sum()
    v = num / den if den > 0 else float("nan")
    return (math.sqrt(v) if np.isfinite(v) and v > 0 else sigma), c1, mu1


def iterate(x, p, w, sigma, c, mu, dense=None):
    """One ECM step: ((sigma, C, mean) of the next model, log-likelihood of THIS model)."""
    e = estep(x, p, w, sigma, c, mu, dense)
    return mstep(sigma, c, mu, e), e["scalars"][1]


def reconstruct(x, p, c, mu, z, mode):
    s = mu + z @ c.T
    return np.where(observed(x, p), x, s) if mode == 1 else s


def subspace_angle(a, b):
    """The largest principal angle between the column spaces of a and b, in degrees."""
    qa, qb = np.linalg.qr(a)[0], np.linalg.qr(b)[0]
    s = np.linalg.svd(qa.T @ qb, compute_uv=False)
    return float(np.degrees(np.arccos(np.clip(s.min(), -1.0, 1.0))))


def case(n, d, k, seed, lo=2.0 ** -10, hi=2.0 ** 10):
    """(x, p, w, (sigma, C, mean)): 30 % of x masked; precisions log-uniform in [lo, hi] with a further 10 % set to 0 and 5 % to NaN,
    independently of x's mask; weights in [0.5, 2], some exactly 0 (n >= 20); the model is near the one the rows were drawn from."""
    rng = np.random.default_rng(seed)
    c_true, mu_true = rng.standard_normal((d, k)), rng.standard_normal(d)
    p = np.exp(rng.uniform(math.log(lo), math.log(hi), (n, d)))
    x = rng.standard_normal((n, k)) @ c_true.T + mu_true + 0.5 * rng.standard_normal((n, d)) / np.sqrt(p)
    x[rng.random((n, d)) < 0.3] = np.nan
    u = rng.random((n, d))
    p[u < 0.10] = 0.0
    p[(u >= 0.10) & (u < 0.15)] = np.nan
    w = rng.uniform(0.5, 2.0, n)
    if n >= 20:
        w[rng.permutation(n)[:max(1, n // 50)]] = 0.0
    return x, p, w, (0.6, 0.7 * c_true + 0.3 * rng.standard_normal((d, k)), mu_true + 0.3 * rng.standard_normal(d))


# The case that justifies the feature: a known k = 3 subspace at d = 12, N = 600, 30 % masked, each entry's noise level drawn from
# {0.3, 3.0} and its precision set to 1 / level^2 (sigma = 1 is the scale).  Thirty iterations from the same random start.
HETERO = dict(n=600, d=12, k=3, seed=4, start_seed=104, levels=(0.3, 3.0), iters=30)


def hetero_case():
    """(x, p, C_true, the random start's transform); the start is (sigma = 1, that transform, mean = 0)."""
    q = HETERO
    rng = np.random.default_rng(q["seed"])
    c, mu = rng.standard_normal((q["d"], q["k"])), rng.standard_normal(q["d"])
    lev = np.asarray(q["levels"])[rng.integers(0, 2, (q["n"], q["d"]))]
    x = rng.standard_normal((q["n"], q["k"])) @ c.T + mu + lev * rng.standard_normal((q["n"], q["d"]))
    x[rng.random(x.shape) < 0.3] = np.nan
    return x, 1.0 / (lev * lev), c, np.random.default_rng(q["start_seed"]).standard_normal(c.shape)


# What this restatement gives on hetero_case(): the largest principal angle to the true subspace, in degrees, with the true precisions
# and with every precision 1 (tests/test_hppca_host.py recomputes both).  The GPU test asks for half the gap between them.
HETERO_ANGLES = (4.4839, 19.5909)
