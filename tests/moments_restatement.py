"""The pairwise second moments of a masked dataset restated in plain numpy, row by row (nothing of the library): what
ppca_dataset_pairwise_moments (include/ppca_hip.h) computes, and the weighted column means `Dataset.pairwise_moments` centres on."""
import numpy as np


def column_means(x, w=None):
    """Weighted means over the observed (finite) entries of every column; 0 for a column with none."""
    n, d = x.shape
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    tot, s = np.zeros(d), np.zeros(d)
    for i in range(n):
        o = np.isfinite(x[i])
        tot[o] += w[i]
        s[o] += w[i] * x[i, o]
    return np.where(tot > 0.0, s / np.where(tot > 0.0, tot, 1.0), 0.0)


def moments(x, w=None, center=None):
    """(sums, counts, cross), d x d each: sum_i w_i x~_ij x~_il, sum_i w_i m_ij m_il, sum_i w_i x~_ij m_il with x~ = x - center on
    observed entries and 0 on masked ones (masked entries are selected out, never multiplied)."""
    n, d = x.shape
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    b = np.zeros(d) if center is None else np.asarray(center, dtype=np.float64)
    sums, counts, cross = np.zeros((d, d)), np.zeros((d, d)), np.zeros((d, d))
    for i in range(n):
        o = np.isfinite(x[i])
        m = o.astype(np.float64)
        xt = np.zeros(d)
        xt[o] = x[i, o] - b[o]
        sums += w[i] * np.outer(xt, xt)
        counts += w[i] * np.outer(m, m)
        cross += w[i] * np.outer(xt, m)
    return sums, counts, cross
