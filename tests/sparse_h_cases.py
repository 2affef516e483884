"""Inputs of the known-precision tests on row-compressed data (tests/test_sparse_h_host.py, tests/test_gpu_sparse_h.py; DESIGN.md
section 4.30).  No test lives here.

The data are those of sparse_cases.case(n, d, k): long-tailed row lengths, row 0 full, empty rows, column 3 with one entry, column 5
with none, column 7 everywhere, one weight 0; the model is the case's scoring model.  Every stored entry gets a precision drawn
log-uniform in [2^-10, 2^10] from default_rng(9000 + 31 n + 7 d + k).  The seam shape forces the row lengths at which the row pass
changes its group width (SEAM_ROWS).  The reference is hppca_restatement.estep / mstep on the dense form with NaN (its k x k form
beyond d = 64, its default)."""
import functools
import math

import numpy as np

import hppca_restatement as R
import sparse_cases as SC
import sparse_fa_cases as F
import state_size_cases as S

SHAPES = [(1, 1, 1), (64, 9, 3), (257, 300, 1), (300, 2000, 10), (150, 300, 11), (200, 1500, 16), (40, 70000, 3)]  # tests/test_gpu_sparse.py's
SWEEP_TILING, SEAM, SEAM_TILINGS = F.SWEEP_TILING, F.SEAM, F.SEAM_TILINGS
SEAM_ROWS = [300, 0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65]  # rows 0 .. 11 of the seam shape: the bins of the row pass change at 16 and 64
SEAM_COLUMNS = (0, 1, 7, 8, 9, 17)  # entries of a column within a block of 64 rows (segment = 8) that the seam shape must show
KS = list(range(1, 17))
# every (n, d, k, tiling) the GPU comparisons run: the shapes at the default tiling, the state-size sweep and the seam shape
CASES = ([(n, d, k, {}) for n, d, k in SHAPES] + [(*S.SPARSE, k, SWEEP_TILING) for k in KS] + [(*SEAM, t) for t in SEAM_TILINGS])
MONOTONE = [(300, 300, 4), (150, 300, 11), (64, 9, 3)]
LO, HI = 2.0 ** -10, 2.0 ** 10


def case_id(c):
    n, d, k, t = c
    return "%dx%dx%d" % (n, d, k) + ("" if not t else "-b%s-s%s" % (t.get("block_rows", "def"), t.get("segment", "def")))


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(n, d, k):
    """-> (x dense with NaN, p dense with NaN at the same places, weights, scoring model (sigma, C, mean), p in CSR order).  Shared
    and read-only."""
    seam = (n, d, k) == SEAM
    x, w, (s, c, mu) = SC.case(n, d, k, forced=[m + 3 if 0 < m < d else m for m in SEAM_ROWS] if seam else None)
    if seam:  # (the edge columns of sparse_cases move a row's length by up to 3: drawn longer, cut to the length from the right)
        for i, m in enumerate(SEAM_ROWS[1:], 1):
            x[i, np.flatnonzero(np.isfinite(x[i]))[m:]] = np.nan
    obs = np.isfinite(x)
    rng = np.random.default_rng(9000 + 31 * n + 7 * d + k)
    pv = np.exp(rng.uniform(math.log(LO), math.log(HI), int(obs.sum())))
    p = np.full(x.shape, np.nan)
    p[obs] = pv  # (row-major: the order of the CSR values)
    _freeze(x, p, w, c, mu, pv)
    return x, p, w, (s, c, mu), pv


@functools.lru_cache(maxsize=None)
def want(n, d, k):
    """hppca_restatement.estep of the case.  Shared and read-only."""
    x, p, w, (s, c, mu), _ = case(n, d, k)
    e = R.estep(x, p, w, s, c, mu)
    _freeze(*[v for v in e.values()], *e["abs"].values())
    return e


# The case that justifies the feature, made sparse: hppca_restatement's two-noise-level case at N = 600, d = 60, k = 3 with 20 % of the
# entries kept, noise levels {0.3, 3.0}, precisions 1 / level^2 (sigma = 1 is the scale).  Thirty steps from the same random start.
HETERO = dict(n=600, d=60, k=3, seed=4, start_seed=104, levels=(0.3, 3.0), keep=0.2, iters=30)
# what hppca_restatement gives on it: the largest principal angle to the true subspace, in degrees, with the true precisions and
# with every precision 1 (tests/test_sparse_h_host.py recomputes both)
HETERO_ANGLES = (4.04, 26.78)


@functools.lru_cache(maxsize=None)
def hetero_case():
    """(x, p, C_true, the random start's transform); the start is (sigma = 1, that transform, mean = 0)."""
    q = HETERO
    rng = np.random.default_rng(q["seed"])
    c, mu = rng.standard_normal((q["d"], q["k"])), rng.standard_normal(q["d"])
    lev = np.asarray(q["levels"])[rng.integers(0, 2, (q["n"], q["d"]))]
    x = rng.standard_normal((q["n"], q["k"])) @ c.T + mu + lev * rng.standard_normal((q["n"], q["d"]))
    gone = rng.random(x.shape) >= q["keep"]
    x[gone] = np.nan
    p = 1.0 / (lev * lev)
    p[gone] = np.nan
    start = np.random.default_rng(q["start_seed"]).standard_normal(c.shape)
    _freeze(x, p, c, start)
    return x, p, c, start


def restatement_angles():
    """The two angles of HETERO_ANGLES, recomputed: thirty restatement steps with the true precisions and with every precision 1."""
    x, p, c_true, start = hetero_case()
    out = []
    for prec in (p, np.where(np.isfinite(x), 1.0, np.nan)):
        model = (1.0, start.copy(), np.zeros(x.shape[1]))
        for _ in range(HETERO["iters"]):
            model, _ = R.iterate(x, prec, None, *model, dense=False)
        out.append(R.subspace_angle(model[1], c_true))
    return tuple(out)
