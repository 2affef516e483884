"""Inputs of the mixture tests on a SparseDataset (tests/test_sparse_mix_host.py, tests/test_gpu_sparse_mix.py).

mix_case(n, d, k, nm): the pattern of sparse_cases (long-tailed row lengths, row 0 full, the empty rows, the edge columns); nm true
models from sparse_cases.true_model, each mean moved by 3 N(0, I); a uniform label per row and the row sampled from its component;
weights 0.5 + U, all positive (the oracle's mix_iterate refuses a weight that is not > 0); the scoring components are the true ones
perturbed (sparse_cases.scoring_model); log_weights = ln Dirichlet(5, ..., 5).  Under the oracle, 9, 6, 17, 22, 21 and 26 % of the rows
of the six SHAPES have a largest posterior below 0.99 (test_sparse_mix_host.py prints the shares and asserts each within 5 % to 60 %):
the responsibilities are exercised, not saturated."""
import numpy as np

import sparse_cases as SC

SHAPES = [(64, 9, 3, 2), (257, 300, 1, 3), (300, 2000, 10, 3), (150, 300, 11, 2), (200, 1500, 16, 2), (300, 300, 4, 8)]
IDS = ["%dx%dx%d-nm%d" % s for s in SHAPES]


def mix_case(n, d, k, nm, forced=None, edit=None):
    """-> (x dense with NaN, weights, (sigmas (nm), cs (nm, d, k), means (nm, d)), log_weights (nm), labels).  forced: sparse_cases.pattern's;
    edit(obs, rng): changes the finished pattern in place (the seams)."""
    rng = np.random.default_rng(9000 + n + d + k + nm)
    obs = SC.edge_columns(SC.pattern(n, d, k, rng, forced))
    if edit is not None:
        edit(obs, rng)
    true = []
    for _ in range(nm):
        s, c, mu = SC.true_model(d, max(k, 1), rng)
        true.append((s, c, mu + 3.0 * rng.standard_normal(d)))
    labels = rng.integers(0, nm, n)
    x = np.full((n, d), np.nan)
    for c, model in enumerate(true):
        rows = np.flatnonzero(labels == c)
        x[rows] = SC.sample(obs[rows], model, rng)
    w = 0.5 + rng.random(n)
    scoring = [SC.scoring_model(model, rng) for model in true]
    sigmas = np.array([m[0] for m in scoring])
    cs = np.stack([m[1] for m in scoring])
    means = np.stack([m[2] for m in scoring])
    if k == 0:
        cs = np.zeros((nm, d, 0))
    log_weights = np.log(rng.dirichlet(np.full(nm, 5.0)))
    return x, w, (sigmas, cs, means), log_weights, labels
