"""Numpy restatement of held-out scoring under the Student-t and the known-precision models and of the K-fold rule,
shared by tests/test_heldout_families_host.py and tests/test_gpu_heldout_families.py.  No test lives here and nothing of the library is
used.  Built on heldout_restatement (the uniforms, summarize, the Gaussian posteriors), hppca_restatement.row and
tppca_restatement.estep; the chain-rule references are those files' DENSE m x m log-densities, which share nothing with the k x k
posterior forms the scores are made of."""
import math

import numpy as np

import heldout_restatement as H
import hppca_restatement as HP
import tppca_restatement as TP

LN_2PI = H.LN_2PI


# ------------------------------------------------------------------ known precisions
def h_entry_scores(train, train_prec, held, held_prec, sigma, c, mean, dense=None):
    """Per entry (n, d), NaN where (held, held_prec) is not observed: e = x - (mean_j + c_j . z), v = sigma^2 / q + c_j^T Sigma c_j,
    l = -1/2 (ln 2 pi + ln v + e^2 / v), with (z, Sigma) of hppca_restatement.row on the row's (train, train_prec)."""
    n, d = held.shape
    dense = d <= 64 if dense is None else dense
    e, v, l = (np.full((n, d), np.nan) for _ in range(3))
    for i in range(n):
        _, z, sig, _ = HP.row(train[i], train_prec[i], sigma, c, mean, dense)
        o = HP.observed(held[i], held_prec[i])
        if not o.any():
            continue
        co = c[o]
        e[i, o] = held[i, o] - (mean[o] + co @ z)
        v[i, o] = sigma * sigma / held_prec[i, o] + np.einsum("ja,ab,jb->j", co, sig, co)
        l[i, o] = -0.5 * (LN_2PI + np.log(v[i, o]) + e[i, o] ** 2 / v[i, o])
    return e, v, l


def h_score(train, train_prec, held, held_prec, sigma, c, mean, w=None):
    return H.summarize(*h_entry_scores(train, train_prec, held, held_prec, sigma, c, mean), w=w)


def h_chain(train, train_prec, held, held_prec, sigma, c, mean):
    """Per held entry (NaN elsewhere): ell(train row with the entry put in at its held precision) - ell(train row), both the dense
    log-density of hppca_restatement.row."""
    out = np.full(held.shape, np.nan)
    for i, j in zip(*np.nonzero(HP.observed(held, held_prec))):
        x, p = train[i].copy(), train_prec[i].copy()
        base = HP.row(x, p, sigma, c, mean, True)[0]
        x[j], p[j] = held[i, j], held_prec[i, j]
        out[i, j] = HP.row(x, p, sigma, c, mean, True)[0] - base
    return out


# ------------------------------------------------------------------ Student-t
def pred_table(d, nu):
    """tbl[m] = ln Gamma((nu_m + 1) / 2) - ln Gamma(nu_m / 2) - 1/2 ln(nu_m pi), nu_m = nu + m, m = 0 .. d"""
    return np.array([math.lgamma(0.5 * (nu + m + 1)) - math.lgamma(0.5 * (nu + m)) - 0.5 * math.log((nu + m) * math.pi)
                     for m in range(d + 1)])


def t_entry_scores(train, held, sigma, c, mean, nu, post=None):
    """Per entry (n, d), NaN where held is not finite: e = x - (mean_j + c_j . z); v = the predictive VARIANCE s nu_m / (nu_m - 2), +inf
    where nu_m <= 2 (such an entry adds 0 to the z^2 sum); l = tbl[m] - 1/2 ln s - 1/2 (nu_m + 1) log1p(e^2 / (nu_m s)) with
    s = (sigma^2 + c_j^T Sigma c_j) (nu + delta) / nu_m.  m, delta (k x k form) and z are tppca_restatement.estep's of `train`, Sigma
    heldout_restatement.posteriors' (or those of `post` = (states, covs))."""
    r = TP.estep(train, None, sigma, c, mean, nu, dense=False)
    states, covs = post if post is not None else H.posteriors(train, sigma, c, mean)
    if post is None:
        states = r["z"]
    num = nu + r["m"].astype(np.float64)
    tbl = pred_table(train.shape[1], nu)[r["m"]]
    fin = np.isfinite(held)
    vg = sigma * sigma + np.einsum("ja,nab,jb->nj", c, covs, c)
    s = np.where(fin, vg * ((nu + r["delta"]) / num)[:, None], np.nan)
    e = np.where(fin, held - (mean[None, :] + states @ c.T), np.nan)
    l = tbl[:, None] - 0.5 * np.log(s) - 0.5 * (num[:, None] + 1.0) * np.log1p(e * e / (num[:, None] * s))
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(num > 2.0, num / (num - 2.0), np.inf)[:, None] * s
    return e, var, l


def t_score(train, held, sigma, c, mean, nu, w=None, post=None):
    return H.summarize(*t_entry_scores(train, held, sigma, c, mean, nu, post=post), w=w)


def t_chain(train, held, sigma, c, mean, nu):
    """Per held entry (NaN elsewhere): ell(train row with the entry put in) - ell(train row), both the dense t log-density of
    tppca_restatement.estep."""
    out = np.full(held.shape, np.nan)
    base = TP.llks(train, sigma, c, mean, nu, dense=True)
    for i, j in zip(*np.nonzero(np.isfinite(held))):
        x = train[i:i + 1].copy()
        x[0, j] = held[i, j]
        out[i, j] = TP.llks(x, sigma, c, mean, nu, dense=True)[0] - base[i]
    return out


# ------------------------------------------------------------------ folds
def fold_edges(n_folds):
    """The n_folds + 1 edges f / n_folds, the last exactly 1.0."""
    return [f / n_folds for f in range(n_folds)] + [1.0]


def holdout_range(x, lo, hi, seed, row_offset=0):
    """heldout_restatement.holdout with the held entries those of lo <= u < hi."""
    x = np.asarray(x, dtype=np.float64)
    obs = np.isfinite(x)
    u = H.holdout_uniforms(x.shape[0], x.shape[1], seed, row_offset)
    hold = obs & (u >= lo) & (u < hi)
    train, held = np.full_like(x, np.nan), np.full_like(x, np.nan)
    train[obs & ~hold] = x[obs & ~hold]
    held[hold] = x[hold]
    return train, held, (int((obs & ~hold).sum()), int(hold.sum()))


def kfold(x, n_folds, seed, row_offset=0):
    e = fold_edges(n_folds)
    return [holdout_range(x, lo, hi, seed, row_offset) for lo, hi in zip(e, e[1:])]
