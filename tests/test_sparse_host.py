"""CPU-only: the host side of SparseDataset -- the inverted-index build against numpy's stable argsort, the
input validation (Python's, before the library is touched, and the library's own, before any device work), the constructors' round
trips and the C-ABI table."""
import ctypes as C

import numpy as np
import pytest

import sparse_cases as SC

INVALID = -1


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _transpose(hiplib, n, d, indptr, indices, values, block_rows):
    nnz = int(indptr[-1])
    br = block_rows if block_rows > 0 else n
    blocks = (n + br - 1) // br if n else 0
    cp = np.full((max(blocks, 1), d + 1), -1, dtype=np.int64)
    trow = np.full(max(nnz, 1), -1, dtype=np.int32)
    tval = np.full(max(nnz, 1), np.nan)
    rc = hiplib.ppca_sparse_transpose_host(n, d, _ptr(indptr), _ptr(indices), _ptr(values), block_rows, _ptr(cp), _ptr(trow), _ptr(tval))
    return rc, cp[:blocks], trow[:nnz], tval[:nnz]


@pytest.mark.parametrize("n,d,k", [(64, 9, 3), (257, 300, 1), (300, 2000, 10), (1, 1, 1)])
def test_transpose_matches_stable_argsort(hiplib, n, d, k):
    x, _, _ = SC.case(n, d, k)
    indptr, indices, values = SC.csr_of(x)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    for br in (1, 7, n):
        rc, cp, trow, tval = _transpose(hiplib, n, d, indptr, indices, values, br)
        assert rc == 0
        for b, r0 in enumerate(range(0, n, br)):
            r1 = min(n, r0 + br)
            e0, e1 = indptr[r0], indptr[r1]
            order = np.argsort(indices[e0:e1], kind="stable")
            assert np.array_equal(trow[e0:e1], (rows[e0:e1][order] - r0).astype(np.int32)), (br, b)
            assert np.array_equal(tval[e0:e1], values[e0:e1][order]), (br, b)
            want = np.concatenate([[0], np.cumsum(np.bincount(indices[e0:e1], minlength=d))])
            assert np.array_equal(cp[b], want), (br, b)


def _good():
    indptr = np.array([0, 2, 2, 5], dtype=np.int64)
    indices = np.array([1, 3, 0, 2, 3], dtype=np.int32)
    values = np.arange(5, dtype=np.float64)
    return indptr, indices, values, 4


BAD = {
    "unsorted column": lambda ip, ix, v, d: (ip, np.array([3, 1, 0, 2, 3], dtype=np.int32), v, d, None),
    "duplicate column": lambda ip, ix, v, d: (ip, np.array([1, 1, 0, 2, 3], dtype=np.int32), v, d, None),
    "column = d": lambda ip, ix, v, d: (ip, np.array([1, 4, 0, 2, 3], dtype=np.int32), v, d, None),
    "negative column": lambda ip, ix, v, d: (ip, np.array([-1, 3, 0, 2, 3], dtype=np.int32), v, d, None),
    "non-monotone indptr": lambda ip, ix, v, d: (np.array([0, 3, 2, 5], dtype=np.int64), ix, v, d, None),
    "indptr not from 0": lambda ip, ix, v, d: (np.array([1, 2, 2, 5], dtype=np.int64), ix, v, d, None),
    "indptr end != nnz": lambda ip, ix, v, d: (np.array([0, 2, 2, 4], dtype=np.int64), ix, v, d, None),
    "NaN value": lambda ip, ix, v, d: (ip, ix, np.array([0, 1, np.nan, 3, 4.0]), d, None),
    "inf value": lambda ip, ix, v, d: (ip, ix, np.array([0, 1, np.inf, 3, 4.0]), d, None),
    "wrong weights length": lambda ip, ix, v, d: (ip, ix, v, d, np.ones(4)),
    "no columns": lambda ip, ix, v, d: (ip, ix, v, 0, None),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_rejected_inputs_raise_value_error(what):
    import ppca_rs_amd as P

    ip, ix, v, d, w = BAD[what](*_good())
    with pytest.raises(ValueError):
        P.SparseDataset(ip, ix, v, d, w)


def test_good_input_needs_no_device():
    import ppca_rs_amd as P

    ip, ix, v, d = _good()
    sp = P.SparseDataset(ip, ix, v, d, [1.0, 2.0, 0.0])
    assert len(sp) == 3 and sp.output_size() == 4 and sp.nnz == 5 and sp.empty_dimensions() == []
    assert np.array_equal(sp.weights(), [1.0, 2.0, 0.0])
    with pytest.raises(ValueError):
        sp.with_weights(np.ones(2))
    with pytest.raises(ValueError):
        P.SparseDataset(ip, ix, v, d, block_rows=0)
    assert len(P.SparseDataset([0], [], [], 3)) == 0 and P.SparseDataset([0], [], [], 3).output_size() is None


@pytest.mark.parametrize("what", ["unsorted column", "duplicate column", "column = d", "non-monotone indptr", "NaN value"])
def test_library_rejects_before_any_device_work(hiplib, what):
    ip, ix, v, d, _ = BAD[what](*_good())
    rc, _, _, _ = _transpose(hiplib, len(ip) - 1, d, np.ascontiguousarray(ip), np.ascontiguousarray(ix), np.ascontiguousarray(v, dtype=np.float64), 0)
    assert rc == INVALID
    assert hiplib.ppca_last_error()


def test_round_trips():
    import ppca_rs_amd as P

    x, w, _ = SC.case(64, 9, 3)
    x[3, 2] = np.inf  # dropped like a NaN
    sp = P.SparseDataset.from_dense(x, w)
    indptr, indices, values = sp.csr()
    want = SC.csr_of(np.where(np.isfinite(x), x, np.nan))
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float64
    assert all(np.array_equal(a, b) for a, b in zip((indptr, indices, values), want))
    assert np.array_equal(sp.weights(), w) and sp.nnz == np.isfinite(x).sum()
    back = sp._dense()
    assert np.array_equal(np.isfinite(back), np.isfinite(x)) and np.array_equal(back[np.isfinite(x)], x[np.isfinite(x)])
    assert sp.empty_dimensions() == [j for j in range(9) if not np.isfinite(x[:, j]).any()] and 5 in sp.empty_dimensions()

    # triplets in any order
    rows = np.repeat(np.arange(64), np.diff(indptr))
    perm = np.random.default_rng(0).permutation(values.size)
    coo = P.SparseDataset.from_coo(rows[perm], indices[perm], values[perm], (64, 9))
    assert all(np.array_equal(a, b) for a, b in zip(coo.csr(), (indptr, indices, values)))
    with pytest.raises(ValueError):
        P.SparseDataset.from_coo([0, 0], [1, 1], [1.0, 2.0], (2, 3))
    with pytest.raises(ValueError):
        P.SparseDataset.from_coo([2], [1], [1.0], (2, 3))

    # csr() hands out copies; the constructor keeps its own
    indptr[1] = -5
    assert sp.csr()[0][1] != -5
    again = P.SparseDataset(*sp.csr(), 9)
    assert all(np.array_equal(a, b) for a, b in zip(again.csr(), sp.csr()))


def test_dense_only_calls_say_so():
    import ppca_rs_amd as P

    sp = P.SparseDataset(*_good()[:3], 4)
    model = P.PPCAModel(1.0, np.ones((4, 2)), np.zeros(4))
    for call in (model.smooth, model.extrapolate):
        with pytest.raises(TypeError, match="predict"):
            call(sp)
    with pytest.raises(ValueError, match="pca"):
        P.PPCAModel.init(2, sp, method="pca")
    with pytest.raises(ValueError):
        model.predict(sp, ([0, 1, 1], [0]))  # a row short
    with pytest.raises(ValueError):
        model.predict(sp, ([0, 1, 1, 2], [0, 4]))  # column = d
    init = P.PPCAModel.init(2, P.SparseDataset([0, 1, 2], [0, 2], [1.0, 2.0], 4), seed=1)
    assert not init.transform[[1, 3]].any() and init.transform[[0, 2]].all()


def test_abi_table_has_the_sparse_symbols(hiplib):
    import test_abi
    from ppca_rs_amd import _lib

    names = [n for n in test_abi._declared_symbols() if n.startswith("ppca_sparse_")]
    assert len(names) == 16 and hiplib.ppca_abi_version() == 6
    for n in names:
        assert hasattr(hiplib, n) and n in _lib.SIGNATURES
    test_abi.test_header_symbols_exported(hiplib)
