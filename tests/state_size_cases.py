"""Inputs of the state-size sweeps (tests/test_state_sizes_host.py and the `state_size_sweep` tests of the GPU files).  No test lives
here.

Almost every hot kernel is compiled once per state size k, so every sweep runs one small case per k.  Every dense case ends its first
rows on the rank edge: rows 0 .. k + 2 hold exactly 0, 1, ..., k + 2 observed entries (capped at d) at random columns -- the rule of
mask_patterns.patterns()["rank_edge"] on the head of the case's own data.  Below k the Gram is rank-deficient and the solve rests on
sigma^2 I.  The row-compressed cases (sparse_cases.case) already hold rows of d, 0, 1, k - 1, k, k + 1 entries.

  family                      shape (n, d)                  k        case
  row-compressed passes       (150, 300)                    0 .. 16  sparse_cases.case
  known-precision model       (130, 97)                     1 .. 16  hetero_case
  Student-t sweep             (70, 40 / 97 / 300)           1 .. 16  robust_case
  split pipeline, lane solver (130, 270)                    1 .. 16  dense_case
  two-kernel shapes           (130, 200)                    11 .. 16 dense_case
  dense mixture step          (300, 40), three components   1 .. 16  mix_case
"""
import numpy as np

import hppca_restatement as HR
import tppca_restatement as TR

KS = tuple(range(1, 17))
SPARSE = (150, 300)
HETERO = (130, 97)
ROBUST_N, ROBUST_DS = 70, (40, 97, 300)
LANE = (130, 270)
TWO_KERNEL, TWO_KERNEL_KS = (130, 200), tuple(range(11, 17))
MIX, MIX_COMPONENTS = (300, 40), 3


def head_counts(n, d, k):
    """The observed counts of the rank-edge head: row r holds min(r, d) entries, r = 0 .. min(k + 2, n - 1)."""
    return np.minimum(np.arange(min(k + 3, n)), d)


def rank_edge_head(x, k, rng, fill):
    """x (NaN = not observed) with rows 0 .. k + 2 replaced: row r keeps min(r, d) entries at random columns -- the row's own values where
    it had them, fill[r, j] elsewhere.  Returns the head's mask."""
    n, d = x.shape
    counts = head_counts(n, d, k)
    head = np.zeros((counts.size, d), dtype=bool)
    for r, m in enumerate(counts):
        head[r, rng.permutation(d)[:m]] = True
    rows = slice(0, counts.size)
    x[rows] = np.where(head, np.where(np.isfinite(x[rows]), x[rows], fill[rows]), np.nan)
    return head


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def hetero_case(k):
    """hppca_restatement.case at (130, 97, k); the head's entries also get finite positive precisions (1 where the case had none), so
    that the restatement's m of row r is exactly r."""
    n, d = HETERO
    seed = 2000 + 31 * n + 7 * d + k
    x, p, w, model = HR.case(n, d, k, seed)
    rng = np.random.default_rng(seed + 1)
    head = rank_edge_head(x, k, rng, model[2] + rng.standard_normal((n, d)))
    rows = slice(0, head.shape[0])
    p[rows] = np.where(head & ~HR.observed(np.zeros_like(p[rows]), p[rows]), 1.0, p[rows])
    _freeze(x, p, w, *model[1:])
    return x, p, w, model


def robust_case(d, k):
    """tppca_restatement.masked_case at (70, d, k) with the head.  (The case's all-masked column d // 3 may gain a head entry.)"""
    n = ROBUST_N
    seed = 1000 + 31 * n + 7 * d + k
    x, w, model = TR.masked_case(n, d, k, seed)
    rng = np.random.default_rng(seed + 1)
    rank_edge_head(x, k, rng, model[2] + rng.standard_normal((n, d)))
    _freeze(x, w, *model[1:])
    return x, w, model


def dense_case(n, d, k):
    """Rows of a k-dimensional model with noise 0.5, 30 % masked, one all-masked row in the body, the head; weights in [0.5, 1.5]; a
    random model to score with and to iterate from (the recipe of tests/test_gpu_parity.py::test_generic_pipeline_matches_oracle)."""
    rng = np.random.default_rng(6000 + 31 * n + 7 * d + k)
    c_true, mu_true = rng.standard_normal((d, k)), rng.standard_normal(d)
    x = rng.standard_normal((n, k)) @ c_true.T + mu_true + 0.5 * rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    x[n // 2] = np.nan
    rank_edge_head(x, k, rng, mu_true + rng.standard_normal((n, d)))
    w = rng.uniform(0.5, 1.5, n)
    c, mu, s = 0.3 * rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d), 0.9
    _freeze(x, w, c, mu)
    return x, w, (s, c, mu)


def mix_case(k):
    """Three components that OVERLAP at (300, 40, k), by the recipe of tests/test_gpu_units.py::_mix_case (close means, loadings around
    a shared one, the models near the generating ones), weighted, one row all masked, with the head.
    -> x, w, (sigmas, transforms, means, log-weights)."""
    (n, d), nm = MIX, MIX_COMPONENTS
    rng = np.random.default_rng(4000 + 17 * d + k)
    parts, cs, ms = [], [], []
    shared = rng.standard_normal((d, k))
    for _ in range(nm):
        c, mu = shared + 0.3 * rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d)
        parts.append(rng.standard_normal((n // nm, k)) @ c.T + mu + 0.5 * rng.standard_normal((n // nm, d)))
        cs.append(c + 0.2 * rng.standard_normal((d, k)))
        ms.append(mu + 0.1 * rng.standard_normal(d))
    x = np.concatenate(parts)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[len(x) // 3] = np.nan
    w = rng.uniform(0.25, 2.0, len(x))
    lw = np.log(rng.dirichlet(5.0 * np.ones(nm)))
    rank_edge_head(x, k, rng, 0.5 * rng.standard_normal((n, d)))
    sig, cs, ms = np.full(nm, 0.5), np.array(cs), np.array(ms)
    _freeze(x, w, sig, cs, ms, lw)
    return x, w, (sig, cs, ms, lw)


def mix_conditions(x, w, log_post):
    """What keeps a mixture case clear of the known finding of DESIGN.md section 7 ("a column that only negligible rows observe"), and
    graded.  -> (the smallest, over the (component, column) pairs, of ln(the largest row weight w_i r_ic among the rows that observe the
    column / the component's largest row weight): the finding needs it below -53 ln 2; the number of rows with two components'
    responsibilities above 1e-6)."""
    with np.errstate(divide="ignore"):
        lr = log_post + np.log(w)[:, None]
    obs = np.isfinite(x)
    best = np.array([[lr[obs[:, j], c].max() if obs[:, j].any() else -np.inf for j in range(x.shape[1])] for c in range(lr.shape[1])])
    return float((best - lr.max(axis=0)[:, None]).min()), int(((np.exp(log_post) > 1e-6).sum(axis=1) >= 2).sum())
