"""Inputs of the factor-analysis tests on row-compressed data (tests/test_sparse_fa_host.py, tests/test_gpu_sparse_fa.py; DESIGN.md
section 4.25).  No test lives here.

fa_case(n, d, k) is sparse_cases.case(n, d, k) in other units per column: column j multiplied by psi_j = 10^U(-1, 1), drawn from
default_rng(8000 + 31 n + 7 d + k), and the scoring model (0.6 psi, psi o C, psi o mean) -- the isotropic scoring model of the case,
noise 0.6, carried into those units.  The pattern is untouched, so the edge rows and columns of sparse_cases stay: row 0 full, the empty
rows, column 3 with one entry, column 5 with none, column 7 everywhere, one weight 0."""
import functools

import numpy as np

import fa_restatement as R
import sparse_cases as SC
import state_size_cases as S

SHAPES = [(1, 1, 1), (64, 9, 3), (257, 300, 1), (300, 2000, 10), (150, 300, 11), (200, 1500, 16), (40, 70000, 3), (100, 20, 0)]
SWEEP_TILING = dict(block_rows=64, segment=8)
SEAM = (300, 300, 4)
SEAM_TILINGS = (dict(block_rows=64, segment=8), dict(block_rows=64), dict(segment=8), dict(block_rows=7, segment=3))
# every (n, d, k, tiling) the GPU comparisons run: the shapes at the default tiling, the state-size sweep and the seam shape
CASES = ([(n, d, k, {}) for n, d, k in SHAPES] + [(*S.SPARSE, k, SWEEP_TILING) for k in range(17)] +
         [(*SEAM, t) for t in SEAM_TILINGS])


def case_id(c):
    n, d, k, t = c
    return "%dx%dx%d" % (n, d, k) + ("" if not t else "-b%s-s%s" % (t.get("block_rows", "def"), t.get("segment", "def")))


def scales(n, d, k):
    return 10.0 ** np.random.default_rng(8000 + 31 * n + 7 * d + k).uniform(-1.0, 1.0, d)


@functools.lru_cache(maxsize=None)
def fa_case(n, d, k):
    """-> (x dense with NaN, weights, scoring model (noise, C, mean), psi).  Shared and read-only."""
    x, w, (s, c, mu) = SC.case(n, d, k)
    psi = scales(n, d, k)
    x = x * psi
    model = (s * psi, c * psi[:, None], mu * psi)
    for a in (x, w, psi) + model:
        a.setflags(write=False)
    return x, w, model, psi


def llks_low_rank(x, psi, c, mu):
    """fa_restatement.llks's quantity -- the log-density of each row under N(mu_O, C_O C_O^T + diag(psi_O^2)) in the ORIGINAL units, no
    whitening of the data -- evaluated through the k x k matrix M = I + C_O^T Psi_O^-2 C_O (the determinant lemma and the Woodbury
    identity).  For the rows the m x m form cannot hold: the full row of the d = 70000 shape would need a 39 GB covariance."""
    out = np.zeros(x.shape[0])
    k = c.shape[1]
    for i, row in enumerate(x):
        o = np.isfinite(row)
        m = int(o.sum())
        if m == 0:
            continue
        r, p2 = row[o] - mu[o], psi[o] ** 2
        cw = c[o] / p2[:, None]
        M = np.eye(k) + cw.T @ c[o]
        b = cw.T @ r
        quad = float(r @ (r / p2)) - (float(b @ np.linalg.solve(M, b)) if k else 0.0)
        logdet = float(np.log(p2).sum()) + (np.linalg.slogdet(M)[1] if k else 0.0)
        out[i] = -0.5 * (quad + logdet + m * R.LN_2PI)
    return out


LONG_ROW = 4000  # entries above which a row's m x m covariance is not formed


def restatement_llks(x, psi, c, mu):
    """fa_restatement.llks on every row it can hold; llks_low_rank on the rows of more than LONG_ROW entries (the host tests hold the
    two to each other on the other shapes)."""
    m = np.isfinite(x).sum(axis=1)
    long = m > LONG_ROW
    out = np.zeros(x.shape[0])
    if (~long).any():
        out[~long] = R.llks(x[~long], psi, c, mu)
    if long.any():
        out[long] = llks_low_rank(x[long], psi, c, mu)
    return out


def whitened_iterate(x, w, psi, c, mu, min_noise=None):
    """fa_restatement.iterate formed in whitened units: the data divided by psi, the model (1, C / psi, mean / psi), one step, and the
    result carried back -- what the device path does."""
    one = np.ones_like(psi)
    floor = None if min_noise is None else min_noise / psi
    p1, c1, m1 = R.iterate(x / psi, w, one, c / psi[:, None], mu / psi, floor)
    return p1 * psi, c1 * psi[:, None], m1 * psi


def zero_variance_columns(x, w, k):
    """The columns whose new noise is 0 in exact arithmetic: without a transform (k = 0) a column with ONE entry of positive weight
    gets that entry as its new mean, and its new variance sq / tot - delta^2 is r^2 - r^2.  What a computation returns there is its
    own rounding: a value <= 0 keeps the old noise (the rule of ppca_fa_finalize_host and of fa_restatement.iterate), a positive one
    gives a noise of at most sqrt(16 u) |r| = 4.3e-8 |r| (u = 2^-53; each of the two squares carries a few roundings).  No relative
    error is defined on such a column, so the comparisons take psi on the others and hold these to `zero_variance_outcome`.  With a
    transform the variance of such a column is a^T Sigma a > 0 and it is compared like every other."""
    if k > 0:
        return np.zeros(x.shape[1], dtype=bool)
    return (np.isfinite(x) & (w[:, None] > 0.0)).sum(axis=0) == 1


def zero_variance_outcome(new_noise, old_noise, x, w, mu, cols, floor=None):
    """True iff on every column of `cols` (zero_variance_columns) the new noise is one of the two outcomes above, under the floor
    where one is given: max(old noise, floor), or a value in [floor, max(floor, 1e-7 |r|)], r = the entry minus the old mean."""
    ok = True
    for j in np.flatnonzero(cols):
        i = int(np.flatnonzero(np.isfinite(x[:, j]) & (w > 0.0))[0])
        tiny = 1e-7 * abs(x[i, j] - mu[j])
        fl = 0.0 if floor is None else float(floor[j])
        ok &= bool(new_noise[j] == max(old_noise[j], fl) or fl <= new_noise[j] <= max(fl, tiny))
    return ok


def model_gaps(got, want, skip=None):
    """(psi relative per element, C per row against max(|c_j|, psi_j), mean against max(|mean_j|, psi_j)): the measures of the issue's
    CPU table.  skip: zero_variance_columns, left out of psi alone."""
    (p1, c1, m1), (p0, c0, m0) = got, want
    crow = np.abs(c1 - c0).max(axis=1) if c0.shape[1] else np.zeros_like(p0)
    cmag = np.maximum(np.abs(c0).max(axis=1) if c0.shape[1] else 0.0, p0)
    keep = np.ones(p0.shape, dtype=bool) if skip is None else ~skip
    perr = float(np.abs(p1 / p0 - 1)[keep].max()) if keep.any() else 0.0
    return perr, float((crow / cmag).max()), float((np.abs(m1 - m0) / np.maximum(np.abs(m0), p0)).max())
