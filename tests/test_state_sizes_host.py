"""The inputs of the state-size sweeps (tests/state_size_cases.py), checked with the references alone (no GPU): the rank-edge head of
every dense case holds the intended counts, the row-compressed shape has rows in all three length bins at every k, the mixture case
meets the two conditions that keep it graded and clear of the dense mixture's known finding, and every reference
output of every case is finite."""
import numpy as np
import pytest

import hppca_restatement as HR
import sparse_cases as SC
import state_size_cases as S
import tppca_restatement as TR


def _finite(*values):
    for v in values:
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(a, dict):
                _finite(a)
            elif isinstance(a, (np.ndarray, float)):
                assert np.isfinite(a).all()


def _assert_head(obs, k):
    n, d = obs.shape
    want = S.head_counts(n, d, k)
    assert want.size == k + 3 and tuple(want) == tuple(range(k + 3))  # (no shape of the sweeps caps a head row)
    assert np.array_equal(obs[:k + 3].sum(axis=1), want)


@pytest.mark.parametrize("k", range(17))
def test_sparse_case(oracle, k):
    n, d = S.SPARSE
    x, w, (s, c, mu) = SC.case(n, d, k)
    lengths = np.isfinite(x).sum(axis=1)
    assert lengths[0] == d - 1 and lengths[1] == 0  # every column but 5; an empty row
    for i, m in enumerate((1, k - 1, k, k + 1)):  # (the edge columns 3, 5 and 7 move a drawn length by at most two)
        assert max(m, 0) - 2 <= lengths[2 + i] <= max(m, 0) + 1
    short, middle, long_ = (lengths <= 16).sum(), ((lengths > 16) & (lengths <= 64)).sum(), (lengths > 64).sum()
    assert short >= 60 and middle >= 24 and long_ >= 28, (short, middle, long_)
    if k:
        _finite(oracle.llks(x, s, c, mu), oracle.llk(x, s, c, mu, w), oracle.infer(x, s, c, mu), oracle.stats(x, s, c, mu, w),
                oracle.iterate(x, s, c, mu, w), oracle.reconstruct(x, s, c, mu, "smooth"))


@pytest.mark.parametrize("k", S.KS)
def test_known_precision_case(k):
    x, p, w, (s, c, mu) = S.hetero_case(k)
    e = HR.estep(x, p, w, s, c, mu)
    assert np.array_equal(e["m"][:k + 3], np.arange(k + 3))
    _assert_head(HR.observed(x, p), k)
    _finite(e, HR.mstep(s, c, mu, e), HR.reconstruct(x, p, c, mu, e["z"], 0))


@pytest.mark.parametrize("d", S.ROBUST_DS)
@pytest.mark.parametrize("k", S.KS)
def test_student_t_case(k, d):
    x, w, (s, c, mu) = S.robust_case(d, k)
    _assert_head(np.isfinite(x), k)
    e = TR.estep(x, w, s, c, mu, 4.0)
    assert np.array_equal(e["m"][:k + 3], np.arange(k + 3))
    _finite(e, TR.mstep(s, c, mu, e))


@pytest.mark.parametrize("shape,k", [(S.LANE, k) for k in S.KS] + [(S.TWO_KERNEL, k) for k in S.TWO_KERNEL_KS],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_dense_case(oracle, shape, k):
    n, d = shape
    x, w, (s, c, mu) = S.dense_case(n, d, k)
    _assert_head(np.isfinite(x), k)
    assert not np.isfinite(x[n // 2]).any()
    _finite(oracle.stats(x, s, c, mu, w), oracle.stats(x, s, c, mu), oracle.llks(x, s, c, mu), oracle.infer(x, s, c, mu),
            oracle.reconstruct(x, s, c, mu, "smooth"), oracle.reconstruct(x, s, c, mu, "extrapolate") [np.isfinite(x)],
            oracle.covariance_diagonal(x, s, c, mu, "smooth"))
    for _ in range(2):
        _finite(oracle.llk(x, s, c, mu, w))
        s, c, mu = oracle.iterate(x, s, c, mu, w)
        _finite(s, c, mu)


@pytest.mark.parametrize("k", S.KS)
def test_mixture_case(oracle, k):
    x, w, (sig, cs, ms, lw) = S.mix_case(k)
    _assert_head(np.isfinite(x), k)
    assert not np.isfinite(x[len(x) // 3]).any()
    post = oracle.mix_infer_cluster(x, sig, cs, ms, lw)
    worst, graded = S.mix_conditions(x, w, post)
    print("k=%d: the best observer of every (component, column) pair at relative log-weight %.3f or above; "
          "%d rows with two components above 1e-6" % (k, worst, graded))
    assert worst >= -53 * np.log(2.0) and graded >= 30
    _finite(oracle.mix_llks(x, sig, cs, ms, lw), post)
    for _ in range(2):
        sig, cs, ms, lw = oracle.mix_iterate(x, sig, cs, ms, lw, w)
        _finite(sig, cs, ms, lw)
