"""CPU-only: the host side of PPCAModel.recommend -- the C-ABI symbol, the argument checks (each raises before
the library or a device is touched) and the restated rule of tests/topn_cases.py against hand-written cases."""
from fractions import Fraction

import numpy as np
import pytest

import sparse_cases as SC
import topn_cases as TC

UNSUPPORTED = -3


def test_abi_has_the_topn_symbol(hiplib):
    import test_abi
    from ppca_rs_amd import _lib

    name = "ppca_topn_sparse"
    assert name in test_abi._declared_symbols() and hasattr(hiplib, name) and name in _lib.SIGNATURES
    test_abi.test_header_symbols_exported(hiplib)


def _sparse_and_model(k=3):
    import ppca_rs_amd as P

    x, w, (s, c, mu) = SC.case(64, 9, 3)
    c = np.random.default_rng(0).standard_normal((9, k))
    return P, P.SparseDataset.from_dense(x, w), P.PPCAModel(s, c, mu)


BAD = {
    "n = 0": dict(n=0),
    "n = 65": dict(n=65),
    "n negative": dict(n=-1),
    "unsorted candidates": dict(n=3, candidates=[0, 4, 2]),
    "repeated candidates": dict(n=3, candidates=[0, 2, 2]),
    "candidate = d": dict(n=3, candidates=[0, 2, 9]),
    "negative candidate": dict(n=3, candidates=[-1, 2]),
    "candidates not integer": dict(n=3, candidates=[0.5, 2.0]),
    "candidates 2-D": dict(n=3, candidates=[[0, 1]]),
    "kappa NaN": dict(n=3, kappa=float("nan")),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_rejected_inputs_raise_before_any_device_work(what):
    P, sp, model = _sparse_and_model()
    with pytest.raises(ValueError):
        model.recommend(sp, **BAD[what])
    assert sp._handle is None and sp._ctx_arg is None and model._dev is None


def test_a_dense_dataset_names_the_constructor():
    P, sp, model = _sparse_and_model()
    with pytest.raises(TypeError, match="SparseDataset.from_dense"):
        model.recommend(P.Dataset.__new__(P.Dataset), 3)
    with pytest.raises(TypeError, match="SparseDataset.from_dense"):
        model.recommend(np.zeros((4, 9)), 3)


def test_state_size_17_is_refused_like_every_sparse_pass():
    P, sp, model = _sparse_and_model(k=17)
    with pytest.raises(P.PPCAError) as err:
        model.recommend(sp, 3)
    assert err.value.code == UNSUPPORTED
    assert sp._handle is None and sp._ctx_arg is None and model._dev is None
    with pytest.raises(ValueError):  # another number of columns
        P.PPCAModel(1.0, np.ones((10, 2)), np.zeros(10)).recommend(sp, 3)


def test_no_rows_give_empty_results_without_a_device():
    import ppca_rs_amd as P

    cols, scores = P.PPCAModel(1.0, np.ones((3, 2)), np.zeros(3)).recommend(P.SparseDataset([0], [], [], 3), 4, candidates=[])
    assert cols.shape == scores.shape == (0, 4) and cols.dtype == np.int32 and scores.dtype == np.float64


# ------------------------------------------------------------------ the restated rule
def test_reference_on_hand_written_cases():
    s = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5],
                  [0.0, -0.0, 7.0, 7.0, 1.0, 1.0]])
    obs = np.array([[0, 0, 1, 0, 0, 0],
                    [0, 0, 0, 1, 0, 0]], dtype=bool)
    # ties go to the lower column; -0.0 and 0.0 tie
    cols, out = TC.topn_reference(s, None, 4)
    assert cols.tolist() == [[1, 2, 4, 0], [2, 3, 4, 5]] and out.tolist() == [[3.0, 3.0, 3.0, 1.0], [7.0, 7.0, 1.0, 1.0]]
    assert cols.dtype == np.int32 and out.dtype == np.float64
    # observed positions leave
    cols, out = TC.topn_reference(s, obs, 3)
    assert cols.tolist() == [[1, 4, 0], [2, 4, 5]] and out.tolist() == [[3.0, 3.0, 1.0], [7.0, 1.0, 1.0]]
    # fewer candidates than n: padding at the end
    cols, out = TC.topn_reference(s, obs, 4, candidates=[0, 2, 3])
    assert cols.tolist() == [[0, 3, -1, -1], [2, 0, -1, -1]]
    assert out[0, :2].tolist() == [1.0, -2.0] and out[1, :2].tolist() == [7.0, 0.0] and np.isnan(out[:, 2:]).all()
    cols, out = TC.topn_reference(s, None, 8)
    assert cols[0].tolist() == [1, 2, 4, 0, 5, 3, -1, -1] and cols[1].tolist() == [2, 3, 4, 5, 0, 1, -1, -1] and np.isnan(out[:, 6:]).all()
    # no candidates
    cols, out = TC.topn_reference(s, None, 2, candidates=[])
    assert (cols == -1).all() and np.isnan(out).all() and cols.shape == out.shape == (2, 2)
    # a row that holds every column
    cols, out = TC.topn_reference(s[:1], np.ones((1, 6), dtype=bool), 3)
    assert (cols == -1).all() and np.isnan(out).all()


def test_fma_rounds_once():
    """TC.fma against exact rational arithmetic: random operands, the kappa values of the GPU tests, and products whose low part decides
    a tie of the last addition."""
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.standard_normal(3000), np.full(3000, 1.5), np.full(3000, -1.0), 1.0 + rng.integers(1, 2 ** 26, 1000) * 2.0 ** -26])
    b = np.concatenate([rng.standard_normal(3000), np.sqrt(rng.random(3000) + 0.3), np.sqrt(rng.random(3000) + 0.3),
                        1.0 + rng.integers(1, 2 ** 26, 1000) * 2.0 ** -26])
    c = np.concatenate([rng.standard_normal(9000) * 10.0 ** rng.integers(-3, 4, 9000), 2.0 ** rng.integers(-60, 3, 1000)])
    got = TC.fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert np.array_equal(got, want)
    assert not np.array_equal(a * b + c, want)  # (two roundings do differ somewhere on this set)
    assert TC.fma(1.5, np.array([2.0, 4.0]), 1.0).tolist() == [4.0, 7.0]  # (a scalar kappa broadcasts)
