"""Inputs of the Student-t tests on row-compressed data (tests/test_sparse_t_host.py, tests/test_gpu_sparse_t.py; DESIGN.md section
4.28).  No test lives here.

The data are those of sparse_cases.case(n, d, k): long-tailed row lengths, row 0 full, empty rows, column 3 with one entry, column 5
with none, column 7 everywhere, one weight 0; the model is the case's scoring model.  The reference is tppca_restatement.estep /
mstep on the dense form with NaN (its k x k forms of delta and ln det beyond d = 64, its default)."""
import functools

import numpy as np

import sparse_cases as SC
import sparse_fa_cases as F
import state_size_cases as S
import tppca_restatement as R

SHAPES = [(1, 1, 1), (64, 9, 3), (257, 300, 1), (300, 2000, 10), (150, 300, 11), (200, 1500, 16), (40, 70000, 3)]  # tests/test_gpu_sparse.py's
NUS = (0.7, 4.0, 200.0)
NU = 4.0
SWEEP_TILING, SEAM, SEAM_TILINGS = F.SWEEP_TILING, F.SEAM, F.SEAM_TILINGS
# every (n, d, k, nu, tiling) the GPU comparisons run: the shapes at the default tiling under three nu, the state-size sweep and the
# seam shape
CASES = ([(n, d, k, nu, {}) for n, d, k in SHAPES for nu in NUS] + [(*S.SPARSE, k, NU, SWEEP_TILING) for k in S.KS] +
         [(*SEAM, NU, t) for t in SEAM_TILINGS])
MONOTONE = [(300, 300, 4), (150, 300, 11), (64, 9, 3)]


def case_id(c):
    n, d, k, nu, t = c
    return "%dx%dx%d-nu%g" % (n, d, k, nu) + ("" if not t else "-b%s-s%s" % (t.get("block_rows", "def"), t.get("segment", "def")))


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(n, d, k):
    """-> (x dense with NaN, weights, scoring model (sigma, C, mean)).  Shared and read-only."""
    x, w, (s, c, mu) = SC.case(n, d, k)
    _freeze(x, w, c, mu)
    return x, w, (s, c, mu)


@functools.lru_cache(maxsize=None)
def want(n, d, k, nu):
    """tppca_restatement.estep of the case at nu.  Shared and read-only."""
    x, w, (s, c, mu) = case(n, d, k)
    e = R.estep(x, w, s, c, mu, nu)
    _freeze(*[v for v in e.values()], *e["abs"].values())
    return e


def packed_stats_of_scaled(x, w, sigma, c, mu, u):
    """The packed statistics (include/ppca_hip.h) of PPCAModel(sigma, C, 0) on the scaled dataset y = sqrt(u) (x - mean), in numpy:
    what the EM pass on the values view hands to ppca_t_finalize_host."""
    n, d = x.shape
    k = c.shape[1]
    kp = k * (k + 1) // 2
    y = np.sqrt(u)[:, None] * (x - mu)
    cross, Sp, totals = np.zeros((d, k)), np.zeros((d, kp)), np.zeros(d)
    tri = [(a, b) for a in range(k) for b in range(a + 1)]
    for i in range(n):
        o = np.isfinite(y[i])
        if not o.any():
            continue
        co = c[o]
        M = sigma ** 2 * np.eye(k) + co.T @ co
        z = np.linalg.solve(M, co.T @ y[i, o])
        P = sigma ** 2 * np.linalg.inv(M) + np.outer(z, z)
        cross[o] += w[i] * np.outer(y[i, o], z)
        Sp[o] += w[i] * np.array([P[a, b] for a, b in tri])
        totals[o] += w[i]
    return np.concatenate([cross.ravel(), Sp.ravel(), np.zeros(d * k), np.zeros(d), totals, np.zeros(8)])


def contaminated():
    """The sparse contaminated case: synth_contaminated(600, 60, 3, 0.05, seed=2, mask=0.8) -- 20 % of the entries exist, the shortest
    row has 3 -- and the start (sigma = 1, C = default_rng(102).standard_normal((60, 3)), mean = 0).
    -> (x, C_true, contaminated rows, the start's transform)"""
    x, c, _, bad = R.synth_contaminated(600, 60, 3, 0.05, seed=2, mask=0.8)
    return x, c, bad, np.random.default_rng(102).standard_normal((60, 3))
