"""Numpy restatement of held-out scoring, shared by tests/test_heldout_host.py and tests/test_gpu_heldout.py.  No test
lives here, and nothing of the library is used: the hold-out rule with the counter-based generator restated bit for bit in uint64
(as tests/test_gpu_posterior_sample.py restates the draws), the scores given the rows' posteriors (z, Sigma), the mixture fold and
the mapping of a whitened score back to the units of a factor model."""
import numpy as np

LN_2PI = float(np.log(2.0 * np.pi))
STREAM_HOLDOUT = 8
_U64 = np.uint64


# ------------------------------------------------------------------ the generator
def smix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
    return x ^ (x >> _U64(31))


def row_key(seed, stream, rows):
    with np.errstate(over="ignore"):
        base = smix64(np.array([seed % 2**64], dtype=np.uint64) ^ np.array([(stream * 0xD1342543DE82EF95) % 2**64], dtype=np.uint64))
        return smix64(base + np.asarray(rows, dtype=np.uint64))


def row_words(keys, n_words):
    p = np.arange(n_words, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return smix64(keys[:, None] + p[None, :] * _U64(0xA0761D6478BD642F))


# ------------------------------------------------------------------ the hold-out rule
def holdout_uniforms(n, d, seed, row_offset=0):
    """(n, d): u of entry (i, j) = (word j of row row_offset + i of stream 8 >> 11) 2^-53, in [0, 1)."""
    w = row_words(row_key(seed, STREAM_HOLDOUT, np.arange(row_offset, row_offset + n)), d)
    return (w >> _U64(11)).astype(np.float64) * 2.0 ** -53


def holdout(x, fraction, seed, row_offset=0):
    """(train, held, (kept, held) counts): an observed entry is held iff u < fraction; held -> NaN in train, the value in held; kept the
    other way round; masked (non-finite) -> NaN in both."""
    x = np.asarray(x, dtype=np.float64)
    obs = np.isfinite(x)
    hold = obs & (holdout_uniforms(x.shape[0], x.shape[1], seed, row_offset) < fraction)
    train, held = np.full_like(x, np.nan), np.full_like(x, np.nan)
    train[obs & ~hold] = x[obs & ~hold]
    held[hold] = x[hold]
    return train, held, (int((obs & ~hold).sum()), int(hold.sum()))


# ------------------------------------------------------------------ the scores, given (z, Sigma)
def entry_scores(held, sigma, c, mean, states, covs):
    """Per entry (n, d), NaN where held is not finite: e = x - (mean_j + c_j^T z), v = sigma^2 + c_j^T Sigma c_j,
    l = -1/2 (ln 2 pi + ln v + e^2 / v).  states (n, k), covs (n, k, k): the posterior of each row given its train entries."""
    held = np.asarray(held, dtype=np.float64)
    m = mean[None, :] + states @ c.T
    v = sigma * sigma + np.einsum("ja,nab,jb->nj", c, covs, c)
    fin = np.isfinite(held)
    e = np.where(fin, held - m, np.nan)
    v = np.where(fin, v, np.nan)
    l = -0.5 * (LN_2PI + np.log(v) + e * e / v)
    return e, v, l


def summarize(e, v, l, w=None):
    """dict(per_row (n), totals (6), col_sums (4, d)) from per-entry e, v, l (NaN = not held); `abs`: the same sums of absolute terms
    (the scale of a sum's rounding)."""
    fin = np.isfinite(l)
    n, d = l.shape
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    z = lambda a: np.where(fin, a, 0.0)
    per_row = z(l).sum(axis=1)
    cols = np.stack([(w[:, None] * fin).sum(axis=0), (w[:, None] * z(l)).sum(axis=0), (w[:, None] * z(e * e)).sum(axis=0),
                     (w[:, None] * z(e * e / v)).sum(axis=0)])
    cols_abs = np.stack([cols[0], (w[:, None] * np.abs(z(l))).sum(axis=0), cols[2], cols[3]])
    totals = np.concatenate([cols.sum(axis=1), [float(fin.sum()), float(fin.any(axis=1).sum())]])
    return dict(per_row=per_row, totals=totals, col_sums=cols, col_abs=cols_abs, total_abs=cols_abs.sum(axis=1))


def posteriors(train, sigma, c, mean):
    """(states, covs) of every row given its finite entries: Sigma = sigma^2 (C_o^T C_o + sigma^2 I)^-1, z = Sigma C_o^T (x_o - mean_o)
    / sigma^2; a row with no entry gets the prior (0, I).  k = 0: empty arrays."""
    n, k = train.shape[0], c.shape[1]
    states, covs = np.zeros((n, k)), np.zeros((n, k, k))
    for i, row in enumerate(train):
        o = np.isfinite(row)
        co = c[o]
        minv = np.linalg.inv(co.T @ co + sigma * sigma * np.eye(k))
        covs[i] = sigma * sigma * minv
        states[i] = minv @ (co.T @ (row[o] - mean[o]))
    return states, covs


def score(train, held, sigma, c, mean, w=None, post=None):
    """summarize(entry_scores(...)) with the posteriors of `post` (states, covs) or, by default, this file's own."""
    states, covs = post if post is not None else posteriors(train, sigma, c, mean)
    return summarize(*entry_scores(held, sigma, c, mean, states, covs), w=w)


# ------------------------------------------------------------------ the mixture fold
def mix_entry_scores(held, comps, logpost):
    """comps: per component (e_c, v_c, l_c) as entry_scores gives them; logpost (n, nm): the rows' log posteriors of the components
    given train.  Per entry l = logsumexp_c(lp_c + l_c); with a_c = exp(lp_c) and m_c - x = -e_c: A = sum a_c (m_c - x), V = sum a_c v_c,
    Q = sum a_c (m_c - x)^2; e = -A, variance V + max(Q - A^2, 0).  A component of weight 0 contributes nothing."""
    held = np.asarray(held, dtype=np.float64)
    fin = np.isfinite(held)
    n, d = held.shape
    mx = np.full((n, d), -np.inf)
    for (_, _, l), lp in zip(comps, logpost.T):
        mx = np.maximum(mx, np.where(fin, lp[:, None] + l, -np.inf))
    sm, A, V, Q = (np.zeros((n, d)) for _ in range(4))
    for (e, v, l), lp in zip(comps, logpost.T):
        live = fin & np.isfinite(lp)[:, None]
        a = np.exp(lp)[:, None]
        with np.errstate(invalid="ignore"):
            sm += np.where(live, np.exp(lp[:, None] + l - mx), 0.0)
            A += np.where(live, a * -e, 0.0)
            V += np.where(live, a * v, 0.0)
            Q += np.where(live, a * e * e, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.where(fin, mx + np.log(sm), np.nan)
    e = np.where(fin, -A, np.nan)
    v = np.where(fin, V + np.maximum(Q - A * A, 0.0), np.nan)
    return e, v, l


def _logsumexp(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.squeeze(m, axis) + np.log(np.exp(a - m).sum(axis=axis))


def mix_score(train, held, sigmas, cs, means, log_weights, comp_llks, w=None, posts=None):
    """comp_llks (n, nm): every component's log-likelihood of the train rows (from the oracle, or any restatement); posts: per
    component (states, covs), default this file's own."""
    lw = np.asarray(log_weights, dtype=np.float64)
    joint = comp_llks + (lw - _logsumexp(lw, 0))[None, :]
    logpost = joint - _logsumexp(joint, 1)[:, None]
    comps = []
    for c, (s, cm, mu) in enumerate(zip(sigmas, cs, means)):
        states, covs = posts[c] if posts is not None else posteriors(train, s, cm, mu)
        comps.append(entry_scores(held, s, cm, mu, states, covs))
    return summarize(*mix_entry_scores(held, comps, logpost), w=w)


# ------------------------------------------------------------------ the factor models' mapping
def unwhiten(res, held, noise):
    """A score of the data whitened by the column scales s = noise, in the units of the data: llk_j -= cnt_j ln s_j, se_j *= s_j^2,
    z2_j unchanged; per row minus the sum of ln s_j over its held entries; totals from the column sums in index order."""
    ln = np.log(noise)
    cols = res["col_sums"].copy()
    cols[1] -= cols[0] * ln
    cols[2] *= noise * noise
    fin = np.isfinite(held)
    per_row = res["per_row"] - (fin * ln[None, :]).sum(axis=1)
    totals = np.concatenate([cols.sum(axis=1), res["totals"][4:]])
    cabs = res["col_abs"].copy()
    cabs[1] += cabs[0] * np.abs(ln)
    cabs[2] *= noise * noise
    return dict(per_row=per_row, totals=totals, col_sums=cols, col_abs=cabs, total_abs=cabs.sum(axis=1))


def fa_score(train, held, noise, c, mean, w=None):
    """The factor model's score by composition: both parts divided by noise, the whitened model PPCA(1, C / noise, mean / noise)."""
    return unwhiten(score(train / noise, held / noise, 1.0, c / noise[:, None], mean / noise, w=w), held, noise)


# ------------------------------------------------------------------ the split cases of tests/test_gpu_heldout.py
# (n, d, seed) of the 30 %-masked datasets that the GPU test splits at every fraction of SPLIT_FRACTIONS; tests/test_heldout_host.py
# checks on the CPU that each (seed, shape, fraction) realises a share of held entries within 5 sqrt(f (1 - f) / n_observed) of f.
SPLIT_SHAPES = ((1, 1, 3), (5, 63, 11), (300, 64, 12), (300, 65, 13), (257, 256, 14), (130, 300, 15), (70, 1024, 16))
SPLIT_FRACTIONS = (0.0, 0.1, 0.5, 1.0)


def split_data(n, d, seed):
    """The dataset of a split case: standard normals, 30 % masked (NaN) at random."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    return x
