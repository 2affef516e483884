"""The restated score, the per-row properties and the inputs of the PPCAMix.recommend tests (tests/test_mix_topn_host.py,
tests/test_gpu_mix_topn.py).  Data from sparse_mix_cases.mix_case, the ranking rule and the single rounding of
a * b + c from topn_cases.

mix_score is the library's combination of the components' predictives, step for step: with r_c the row's posterior weights and
(m_c, v_c) component c's predict, mean = r_0 m_0 then fma(r_c, m_c, mean); var likewise from the v_c; s = fma(r_c, (m_c - mean)^2, s)
from 0; score = fma(kappa, sqrt(var + s), mean), or the mean itself at kappa = 0 -- the components in index order."""
import numpy as np

import sparse_cases as SC
import sparse_mix_cases as MC
import topn_cases as TC

TOL = 1e-5  # the project's GPU parity bound, relative to 1 + |value| (tests/test_gpu_topn.py)
KAPPAS = (0.0, 1.5, -1.0)


def mix_moments(means, vars_, post):
    """means, vars_ (nm, N, d); post (N, nm) -> (mean, var + spread), the two values of PPCAMix.predict, rounded as the library rounds."""
    means, vars_ = np.asarray(means, dtype=np.float64), np.asarray(vars_, dtype=np.float64)
    r = np.asarray(post, dtype=np.float64).T[:, :, None]
    mean, var = r[0] * means[0], r[0] * vars_[0]
    for c in range(1, means.shape[0]):
        mean = TC.fma(r[c], means[c], mean)
        var = TC.fma(r[c], vars_[c], var)
    s = np.zeros_like(mean)
    for c in range(means.shape[0]):
        dv = means[c] - mean
        s = TC.fma(r[c], dv * dv, s)
    return mean, var + s


def mix_score(means, vars_, post, kappa):
    mean, var = mix_moments(means, vars_, post)
    return TC.score(mean, var, kappa)


def rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def check_against(cols, scores, want, obs, n_top, label):
    """The five per-row properties of a returned list against reference scores `want` (N, d), candidates = the unobserved columns:
    counts and padding; distinct unobserved columns; order; scores within TOL; the cut-off not missed by more than 2 TOL.
    -> (worst score error, worst miss of the cut-off)."""
    n, d = want.shape
    worst_score, worst_cut = 0.0, -np.inf
    for i in range(n):
        candidates = np.flatnonzero(~obs[i])
        ni = min(n_top, candidates.size)
        ci, si = cols[i], scores[i]
        assert np.all(ci[:ni] >= 0) and np.all(ci[ni:] == -1) and np.all(np.isfinite(si[:ni])) and np.all(np.isnan(si[ni:])), (label, i)
        assert np.unique(ci[:ni]).size == ni and not obs[i, ci[:ni]].any(), (label, i)
        step = np.diff(si[:ni])
        assert np.all(step <= 0) and np.all(np.diff(ci[:ni])[step == 0] > 0), (label, i)
        if ni == 0:
            continue
        worst_score = max(worst_score, rel(si[:ni], want[i, ci[:ni]]))
        cut = np.partition(want[i, candidates], candidates.size - ni)[candidates.size - ni]  # the ni-th largest
        worst_cut = max(worst_cut, float((cut - want[i, ci[:ni]].min()) / (1.0 + abs(cut))))
    worst_cut = max(worst_cut, 0.0)
    print("%s: scores %.1e (bound %g), cut-off missed by %.1e (bound %g)" % (label, worst_score, TOL, worst_cut, 2 * TOL))
    assert worst_score <= TOL and worst_cut <= 2 * TOL, label
    return worst_score, worst_cut


# ------------------------------------------------------------------ shapes (n, d, k, nm)
EXACT = [(64, 9, 3, 2), (257, 300, 1, 3), (150, 300, 11, 2), (300, 300, 4, 8), (120, 200, 16, 3)]
SIZES = [(150, 300, k, 2) for k in range(17)]
MIXED = [((64, 9, 3, 3), (3, 1, 0)), ((150, 300, 11, 2), (10, 11))]  # (the case, the components' state sizes)
MANY = (64, 9, 3, 17)  # one component past MIX_MAX = 16
ONE = [(64, 9, 3, 1), (150, 300, 11, 1)]
ORACLE = [(64, 9, 3, 2), (300, 2000, 10, 3), (200, 1500, 16, 2)]
DETERMINISM = [(40, 70000, 3, 2), (300, 2000, 10, 3)]
SEAM_DS = (1, 63, 64, 65, 129)
SEAM_N = 70  # more than one row tile at either tile height


def seam_lengths(d, n_top=5):
    return tuple(min(max(m, 0), d) for m in (d, d - 1, d - n_top, d - n_top + 1, 0, 1))


def seam_case(d, n_top=5):
    """mix_case at (70, d, 3, nm 2) whose rows 0-5 hold exactly d, d - 1, d - n, d - n + 1, 0 and 1 entries (the rows of
    topn_cases.seam_case; set after the edge columns, which would change them)."""
    want = seam_lengths(d, n_top)

    def edit(obs, rng):
        for i, m in enumerate(want):
            obs[i] = False
            obs[i, rng.choice(d, size=m, replace=False)] = True

    return MC.mix_case(SEAM_N, d, 3, 2, forced=want, edit=edit)


def tie_case():
    """topn_cases.tie_case as a two-component mixture: the second component is the first perturbed, and columns 10, 74, 110 and 199
    carry one row of C and one mean in EVERY component, large enough to lead every row's list.
    -> (x, w, (sigmas, cs, means), log_weights, the tied columns)."""
    x, w, (s, c, mu), same = TC.tie_case()
    rng = np.random.default_rng(77)
    c2, mu2 = c + 0.3 * rng.standard_normal(c.shape), mu + 1.0 * rng.standard_normal(mu.shape)
    c2[same] = c2[same[0]]
    mu2[same] = 48.0
    return x, w, (np.array([s, 0.8]), np.stack([c, c2]), np.stack([mu, mu2])), np.log([0.4, 0.6]), same


def unsaturated_cases():
    """Every mix_case the GPU tests use that is not one of sparse_mix_cases.SHAPES: {label: a call that returns the mix_case}."""
    out = {}
    for shape in EXACT + SIZES + [s for s, _ in MIXED] + [MANY] + ORACLE + DETERMINISM:
        if shape not in MC.SHAPES:
            out["%dx%dx%d-nm%d" % shape] = lambda shape=shape: MC.mix_case(*shape)
    for d in SEAM_DS:
        out["seam-d%d" % d] = lambda d=d: seam_case(d)
    return out
