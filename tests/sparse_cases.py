"""Inputs of the SparseDataset tests (tests/test_sparse_host.py, tests/test_gpu_sparse.py): long-tailed row lengths from a true model,
with the edge rows and columns the passes must get right.

case(n, d, k): row i holds floor(d^u) entries, u uniform in [0, 1), at random columns, drawn from a true model with sigma = 0.5.  Then,
where the shape has room: rows 0-5 get the lengths d, 0, 1, k - 1, k, k + 1; the last row is empty; column 7 is observed in every
non-empty row; column 3 in row 0 only; column 5 never (row 0 therefore has every column but 5); one weight is 0 (n > 1).  The scoring model is
the true one perturbed: C + 0.3 N, mean + 0.2 N, sigma = 0.6."""
import numpy as np


def pattern(n, d, k, rng, forced=None):
    """A boolean (n, d) mask with the rules above; forced: row lengths that replace the rows' draws, from row 0 on."""
    obs = np.zeros((n, d), dtype=bool)
    lengths = np.floor(d ** rng.random(n)).astype(int)
    head = [d, 0, 1, k - 1, k, k + 1] if forced is None else list(forced)
    for i, m in enumerate(head[:n]):
        lengths[i] = min(max(m, 0), d)
    if n > 6:
        lengths[-1] = 0
    for i in range(n):
        obs[i, rng.choice(d, size=min(lengths[i], d), replace=False)] = True
    return obs


def edge_columns(obs):
    n, d = obs.shape
    nonempty = obs.any(axis=1)
    if d > 7 and n > 1:
        obs[nonempty, 7] = True
    if d > 3 and n > 1:
        obs[1:, 3] = False
        obs[0, 3] = True
    if d > 5 and n > 1:
        obs[:, 5] = False
    return obs


def true_model(d, k, rng):
    return 0.5, rng.standard_normal((d, k)), rng.standard_normal(d)


def sample(obs, model, rng):
    sigma, c, mean = model
    n, d = obs.shape
    z = rng.standard_normal((n, c.shape[1]))
    x = z @ c.T + mean + sigma * rng.standard_normal((n, d))
    x[~obs] = np.nan
    return x


def scoring_model(model, rng):
    _, c, mean = model
    return 0.6, c + 0.3 * rng.standard_normal(c.shape), mean + 0.2 * rng.standard_normal(mean.shape)


def case(n, d, k, seed=None, forced=None):
    """-> (x dense with NaN, weights, scoring model (sigma, C, mean))."""
    rng = np.random.default_rng(7000 + 31 * n + 7 * d + k if seed is None else seed)
    obs = edge_columns(pattern(n, d, k, rng, forced))
    model = true_model(d, max(k, 1), rng)
    x = sample(obs, model, rng)
    w = 0.5 + rng.random(n)
    if n > 1:  # (a single row keeps its weight: with none the step is not defined)
        w[n // 2] = 0.0
    s, c, mu = scoring_model(model, rng)
    if k == 0:
        c = np.zeros((d, 0))
    return x, w, (s, c, mu)


def csr_of(x):
    obs = np.isfinite(x)
    indptr = np.concatenate([[0], np.cumsum(obs.sum(axis=1))]).astype(np.int64)
    return indptr, np.nonzero(obs)[1].astype(np.int32), x[obs]
