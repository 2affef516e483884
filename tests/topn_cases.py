"""The restated rule and the inputs of the top-n tests (tests/test_topn_host.py, tests/test_gpu_topn.py).

topn_reference is the rule itself: per row a lexsort by (-score, column) over the candidate set, cut at n and padded.  fma is the one
rounding of a * b + c in numpy (Python 3.10 has no math.fma): the score of the library is fma(kappa, sqrt(var), mean), and a ranking
can only be compared exactly against scores that are rounded the same way."""
import numpy as np

import sparse_cases as SC


def topn_reference(scores, obs, n, candidates=None):
    """scores (N, d); obs (N, d) bool: the positions that are excluded, or None; candidates: None (all) or increasing columns.
    -> (columns int32 (N, n), scores (N, n)), padded at the end with -1 / NaN."""
    scores = np.asarray(scores, dtype=np.float64)
    rows, d = scores.shape
    cand = np.arange(d) if candidates is None else np.asarray(candidates, dtype=np.int64)
    cols, out = np.full((rows, n), -1, dtype=np.int32), np.full((rows, n), np.nan)
    for i in range(rows):
        c = cand if obs is None else cand[~obs[i, cand]]
        s = scores[i, c]
        order = np.lexsort((c, -s))[:n]
        cols[i, :order.size] = c[order]
        out[i, :order.size] = s[order]
    return cols, out


# ------------------------------------------------------------------ a * b + c with one rounding
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a  # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(a, b):
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def fma(a, b, c):
    """round(a * b + c), elementwise, for doubles far from overflow and underflow (Boldo and Melquiond 2008: the product and the two
    sums are exact, the low parts are added with rounding to odd, and the last addition rounds once)."""
    a, b, c = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), np.broadcast(a, b, c).shape)) for v in (a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _round_to_odd_sum(tl, vl)


def score(mean, var, kappa):
    """The library's score from predict's two values."""
    return mean.copy() if kappa == 0 else fma(kappa, np.sqrt(var), mean)


# ------------------------------------------------------------------ inputs
def all_positions(n, d):
    """The query that names every position, for PPCAModel.predict."""
    return np.arange(n + 1, dtype=np.int64) * d, np.tile(np.arange(d, dtype=np.int32), n)


def tie_case():
    """(x, w, model) at (32, 200, 4): columns 10, 74 (= 10 + 64), 110 and 199 carry one row of C and one mean, large enough to lead every
    row's list, and none of them is observed."""
    x, w, (s, c, mu) = SC.case(32, 200, 4)
    x, c, mu = x.copy(), c.copy(), mu.copy()
    same = [10, 74, 110, 199]
    c[same] = c[10]
    mu[same] = 50.0
    x[:, same] = np.nan
    return x, w, (s, c, mu), same


def seam_case(d, n_top=5):
    """N = 70, k = 3 with rows 0-5 of exactly d, d - 1, d - n, d - n + 1, 0 and 1 entries (clipped to [0, d]); no edge columns."""
    rng = np.random.default_rng(400 + d)
    obs = SC.pattern(70, d, 3, rng, forced=(d, d - 1, d - n_top, d - n_top + 1, 0, 1))
    model = SC.true_model(d, 3, rng)
    x = SC.sample(obs, model, rng)
    return x, SC.scoring_model(model, rng)
