"""Data in other units: the exact power-of-two rescaling shared by tests/test_units_host.py and tests/test_gpu_units.py.

Multiplying the data, the mean and the loadings by a = 2^p, and the noise level by a, is exact in binary floating point as long as
nothing overflows or goes subnormal: every product, sum, fused multiply-add, reciprocal square root of an even power and integer
digit cut commutes with it.  So a run on scaled inputs must give

  * bit-identical posteriors, unit-free statistics, z-scores, labels and draws' inputs,
  * everything with units as the unscaled result times an exact power of two (compared after `ldexp`, with `np.array_equal`),
  * log-likelihoods shifted by cnt * p * ln 2, cnt the number of entries the term scores -- the only inexact relation, bounded by
    a derived rounding count (`assert_llk`).

A mismatch in a single bit means an absolute constant, a threshold that is not relative, an overflow or a flush to zero.  The same
holds for the sample weights times 2^q: every statistic scales by exactly 2^q or stays as it is, and the new model is bit-identical.

The reference of a scaled run is the library's own unscaled run (pinned to the oracle by the rest of the suite): the fp64 oracle
takes the logarithm of a literal LU determinant and leaves the finite range at these scales (tests/test_units_host.py shows where).
"""
import math

import numpy as np

LN2 = math.log(2.0)
POWERS = (40, -40)  # 1e+12 and 1e-12
WEIGHT_POWERS = (30, -30)
LLK_ULPS = 16.0

# (n, d, k) by engine: the smallest shapes that still reach each one
FUSED = [(200, 256, 10), (97, 33, 3), (130, 255, 7), (64, 5, 1)]  # em9
TWO_KERNEL = [(130, 200, 16), (100, 255, 11)]  # em16
SPLIT = [(60, 300, 4), (64, 70, 20), (40, 80, 65)]  # the generic pipeline; k = 65: the blocked MFMA solver
K_ZERO = [(50, 9, 0)]
SHAPES = FUSED + TWO_KERNEL + SPLIT + K_ZERO
VARIANTS = ("plain", "weighted", "grid1")


def make_case(n, d, k, seed=0, mean_scale=1.0, mask=0.3):
    """Order-one data with `mask` of the entries masked and one row with nothing observed (`empty`), weights, and a model that is
    not the generating one: dict(x, w, sigma, c, mu, empty)."""
    rng = np.random.default_rng(77_000 + 131 * n + 17 * d + k + seed)
    c_true = rng.standard_normal((d, k))
    mean_true = mean_scale * rng.standard_normal(d)
    x = rng.standard_normal((n, k)) @ c_true.T + mean_true + 0.1 * rng.standard_normal((n, d))
    x[rng.random((n, d)) < mask] = np.nan
    empty = n // 3
    x[empty] = np.nan
    c = 0.5 * rng.standard_normal((d, k))
    mu = mean_true + 0.2 * rng.standard_normal(d)
    return dict(x=x, w=rng.uniform(0.25, 2.0, n), sigma=0.7, c=c, mu=mu, empty=empty)


# --------------------------------------------------------------------------- builders
def pow2(v, p):
    """v * 2^p, exactly (p: an integer or an integer array that broadcasts against v)."""
    return np.ldexp(np.asarray(v, dtype=np.float64), p)


def scaled_data(x, p):
    """The dataset in units 2^p times smaller: every finite entry times 2^p (p an integer, or one per column)."""
    return pow2(x, p)


def scaled_model(sigma, c, mu, p):
    """(sigma a, C a, mu a): the PPCA / t model of the scaled data."""
    return float(np.ldexp(sigma, p)), pow2(c, p), pow2(mu, p)


def scaled_fa(noise, c, mu, p):
    """(noise a, C a, mu a) with a = 2^p per column (p an integer or an integer array of length d)."""
    p = np.asarray(p)
    return pow2(noise, p), pow2(c, p[:, None] if p.ndim else p), pow2(mu, p)


def scaled_columns(c, mu, pj):
    """(C, mu) with row j times 2^pj[j]: the known-precision model of data whose column j is scaled by 2^pj[j]."""
    pj = np.asarray(pj)
    return pow2(c, pj[:, None]), pow2(mu, pj)


def scaled_precisions(prec, pj):
    """Precisions of data whose columns are scaled by 2^pj at a fixed noise level: p_ij * 2^(-2 pj)."""
    return pow2(prec, -2 * np.asarray(pj))


def stat_blocks(d, k):
    """[(name, begin, end)] of the packed statistics (include/ppca_hip.h, ppca_stats_len)."""
    kp = k * (k + 1) // 2
    b = [0, d * k, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d, 2 * d * k + d * kp + 2 * d]
    return list(zip(["cross", "S", "U", "sumx", "totals", "scalars"], b, b[1:] + [b[-1] + 8]))


# scalars: square_error, deviations_square_sum, llk, sum w, #non-empty samples, 0, 0, 0
DATA_POWER = dict(cross=1, S=0, U=0, sumx=1, totals=0)  # units of the data per block
SCALAR_DATA_POWER = (2, 2, None, 0, 0, 0, 0, 0)  # None: the llk relation
WEIGHT_POWER = dict(cross=1, S=1, U=1, sumx=1, totals=1)
SCALAR_WEIGHT_POWER = (1, 1, 1, 1, 0, 0, 0, 0)  # the count of non-empty samples is weight-free


def scaled_stats(stats, d, k, p=0, q=0):
    """The packed statistics of data times 2^p under weights times 2^q, from the unscaled ones: exact in every entry but the llk
    scalar at p != 0, which is returned as NaN (it follows `assert_llk`)."""
    out = np.array(stats, dtype=np.float64)
    for name, a, b in stat_blocks(d, k):
        if name != "scalars":
            out[a:b] = pow2(out[a:b], p * DATA_POWER[name] + q * WEIGHT_POWER[name])
            continue
        for i in range(8):
            dp = SCALAR_DATA_POWER[i]
            if dp is None and p != 0:
                out[a + i] = np.nan
            else:
                out[a + i] = pow2(out[a + i], p * (dp or 0) + q * SCALAR_WEIGHT_POWER[i])
    return out


# --------------------------------------------------------------------------- comparisons
def assert_finite(a, what, where=None):
    a = np.asarray(a, dtype=np.float64)
    sel = a if where is None else a[where]
    assert np.isfinite(sel).all(), ("not finite", what)


def assert_bits(got, want, what, where=None):
    """Bit-equality of two arrays (or scalars), both finite first -- on `where` (a boolean array) when given, and then NaN on both
    sides elsewhere."""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape, ("shape", what, g.shape, w.shape)
    if g.dtype.kind in "iub":
        assert np.array_equal(g, w), (what, "integers differ")
        return
    assert_finite(g, what, where)
    assert_finite(w, what, where)
    if where is not None:
        assert np.isnan(g[~where]).all() and np.isnan(w[~where]).all(), ("outside the compared entries", what)
        g, w = g[where], w[where]
    if not np.array_equal(g, w):
        bad = np.flatnonzero(np.ravel(g != w))
        i = bad[0]
        raise AssertionError((what, "%d of %d entries differ" % (bad.size, g.size), "first", int(i), float(np.ravel(g)[i]), float(np.ravel(w)[i])))


def unscale(got, p):
    """got * 2^-p: the scaled run's output in the units of the unscaled one (exact)."""
    return pow2(got, -np.asarray(p))


def assert_pow2(got, base, p, what, where=None):
    """got == base * 2^p bit for bit (p: an integer power, or an array that broadcasts)."""
    assert_bits(unscale(got, p), base, what, where)


def llk_bound(base, cnt, p):
    """16 * 2^-52 * (|llk| + cnt |p| ln 2): every summand of a Gaussian log-density except pe * LN_2 and (m - k) ln sigma is
    bit-identical under the rescaling, and those two add at most four roundings of the largest term; 16 is a fourfold margin."""
    return LLK_ULPS * 2.0 ** -52 * (np.abs(base) + np.abs(cnt) * abs(p) * LN2)


def log_sum_bound(m, total):
    """The rounding of a Jacobian term sum_j ln(s_j 2^p) that a family takes per entry with a library logarithm and adds up in fp64
    (FAModel, FAMix: the sum of ln noise_j over a row's observed entries): m terms of absolute sum `total`, each logarithm within one
    ulp of its value and the m - 1 additions within (m - 1) u of the absolute sum (Higham, Accuracy and Stability, eq. 4.4), on both the
    scaled and the unscaled side: 2 (m + 1) 2^-53 total."""
    return 2.0 * (np.asarray(m, dtype=np.float64) + 1.0) * 2.0 ** -53 * np.asarray(total, dtype=np.float64)


def assert_llk(got, base, cnt, p, what, extra=0.0):
    """|llk' - (llk - cnt p ln 2)| <= llk_bound (+ extra, a derived rounding bound of a term the family adds, stated at the call),
    element by element; cnt: the number of entries each term scores (weighted where the term is)."""
    got, base, cnt = np.asarray(got, dtype=np.float64), np.asarray(base, dtype=np.float64), np.asarray(cnt, dtype=np.float64)
    assert_finite(got, what)
    assert_finite(base, what)
    err = np.abs(got - (base - cnt * p * LN2))
    bound = llk_bound(base, cnt, p) + extra
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0
    assert np.all(err <= bound), (what, "llk relation off by %.3g of the bound" % worst)


def assert_stats(got, base, d, k, p, q, what, llk_cnt=None, llk_extra=0.0):
    """The packed statistics of the scaled run against the unscaled ones, block by block; the llk scalar by `assert_llk` with
    llk_cnt = sum_i w_i m_i (p != 0; llk_extra: see assert_llk), or as an exact multiple (p == 0)."""
    want = scaled_stats(base, d, k, p, q)
    for name, a, b in stat_blocks(d, k):
        if name == "scalars" and p != 0:
            keep = [i for i in range(8) if i != 2]
            assert_bits(got[a:b][keep], want[a:b][keep], (what, name))
            assert_llk(got[a + 2], pow2(base[a + 2], q), llk_cnt, p, (what, "llk scalar"), llk_extra)
        else:
            assert_bits(got[a:b], want[a:b], (what, name))
