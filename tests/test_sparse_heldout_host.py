"""CPU-only: the hold-out split of row-compressed data -- ppca_heldout_split_csr_host against the restated rule
of tests/heldout_restatement.py (the dense split's words, `lo <= u < hi`), SparseDataset.holdout / holdout_range / kfold built on it
(no device is touched), their argument checks and the two new C-ABI symbols."""
import ctypes as C

import numpy as np
import pytest

import heldout_restatement as H
import sparse_cases as SC

INVALID = -1
OFFSETS = (0, 1000, 2 ** 40)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _split(hiplib, indptr, indices, lo, hi, seed, row_offset):
    nnz = int(indptr[-1])
    flags = np.full(max(nnz, 1), 7, dtype=np.uint8)
    counts = np.full(2, -1, dtype=np.int64)
    rc = hiplib.ppca_heldout_split_csr_host(len(indptr) - 1, _ptr(indptr), _ptr(indices), lo, hi, seed, row_offset, _ptr(flags), _ptr(counts))
    return rc, flags[:nnz], counts


def _entry_uniforms(indptr, indices, seed, row_offset):
    """u of every stored entry, the word computed per entry (no n x d array)."""
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.uint64), np.diff(indptr)) + np.uint64(row_offset)
    keys = H.row_key(seed, H.STREAM_HOLDOUT, rows)
    with np.errstate(over="ignore"):
        w = H.smix64(keys + indices.astype(np.uint64) * np.uint64(0xA0761D6478BD642F))
    return (w >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("f", H.SPLIT_FRACTIONS)
@pytest.mark.parametrize("n,d,seed", H.SPLIT_SHAPES)
def test_split_matches_the_restated_rule(hiplib, n, d, seed, f):
    x = H.split_data(n, d, seed)
    indptr, indices, _ = SC.csr_of(x)
    obs = np.isfinite(x)
    for off in OFFSETS:
        u = H.holdout_uniforms(n, d, seed, off)[obs]  # (row-major, the order of the CSR)
        for lo, hi in ((0.0, f), (f, 1.0)):
            want = (u >= lo) & (u < hi)
            rc, flags, counts = _split(hiplib, indptr, indices, lo, hi, seed, off)
            assert rc == 0 and np.array_equal(flags, want.astype(np.uint8)), (off, lo, hi)
            assert tuple(counts) == (int((~want).sum()), int(want.sum()))


def test_split_of_a_wide_case(hiplib):
    x, _, _ = SC.case(40, 70000, 3)
    indptr, indices, _ = SC.csr_of(x)
    assert indices.max() > 65535
    for off in OFFSETS:
        u = _entry_uniforms(indptr, indices, 21, off)
        for lo, hi in ((0.0, 0.3), (0.3, 0.75)):
            want = (u >= lo) & (u < hi)
            rc, flags, counts = _split(hiplib, indptr, indices, lo, hi, 21, off)
            assert rc == 0 and np.array_equal(flags, want.astype(np.uint8)), (off, lo, hi)
            assert tuple(counts) == (int((~want).sum()), int(want.sum()))
    assert 0 < counts[1] < indices.size


def test_the_per_entry_words_are_the_dense_ones():
    """_entry_uniforms (used for the wide case) against the restatement's n x d table."""
    x = H.split_data(130, 300, 15)
    indptr, indices, _ = SC.csr_of(x)
    assert np.array_equal(_entry_uniforms(indptr, indices, 15, 1000), H.holdout_uniforms(130, 300, 15, 1000)[np.isfinite(x)])


# ------------------------------------------------------------------ SparseDataset.holdout
def _rows_of(sp):
    return np.repeat(np.arange(len(sp)), np.diff(sp._indptr))


def _positions(sp):
    return _rows_of(sp).astype(np.int64) * sp._d + sp._indices


def _check_parts(parent, train, held):
    """train and held are disjoint, strictly increasing within rows, and their union is the parent entry for entry, bit for bit."""
    for part in (train, held):
        assert len(part) == len(parent) and part._d == parent._d
        assert part._indptr.dtype == np.int64 and part._indices.dtype == np.int32 and part._values.dtype == np.float64
        assert part._indptr[0] == 0 and part._indptr[-1] == part._indices.size == part._values.size
        pos = _positions(part)
        assert np.all(np.diff(pos) > 0)  # (rows ascending, columns strictly increasing within a row)
    pt, ph = _positions(train), _positions(held)
    assert np.intersect1d(pt, ph).size == 0
    both = np.concatenate([pt, ph])
    order = np.argsort(both, kind="stable")
    assert np.array_equal(both[order], _positions(parent))
    vals = np.concatenate([train._values, held._values])[order]
    assert np.array_equal(vals.view(np.int64), parent._values.view(np.int64))


@pytest.mark.parametrize("n,d,k", [(64, 9, 3), (257, 300, 1), (1, 1, 1)])
def test_holdout_parts(hiplib, n, d, k):
    import ppca_rs_amd as P

    x, w, _ = SC.case(n, d, k)
    sp = P.SparseDataset.from_dense(x, w, block_rows=64, segment=8)
    indptr, indices, _ = sp.csr()
    for f in (0.0, 0.3, 1.0):
        train, held = sp.holdout(f, 5)
        _check_parts(sp, train, held)
        want = _entry_uniforms(indptr, indices, 5, 0) < f
        assert np.array_equal(_positions(held), _positions(sp)[want])
        assert train.holdout_counts == held.holdout_counts == (int((~want).sum()), int(want.sum()))
        for part in (train, held):
            assert np.array_equal(part.weights(), w) and part._d == d and part._block_rows == 64 and part._segment == 8
            assert part._ctx_arg is sp._ctx_arg
        assert sp._handle is None and train._handle is None and held._handle is None  # no device copy was made
        if f == 0.0:
            assert held.nnz == 0 and train.nnz == sp.nnz
        if f == 1.0:
            assert train.nnz == 0 and held.nnz == sp.nnz
    # the defaults are carried as defaults, and a shard with its offset reproduces its rows of the whole
    plain = P.SparseDataset.from_dense(x)
    t0, h0 = plain.holdout(0.3, 5)
    assert (t0._block_rows, t0._segment, t0._w) == (0, 0, None)
    if n >= 4:
        s0 = n // 3
        ts, hs = P.SparseDataset.from_dense(x[s0:]).holdout(0.3, 5, row_offset=s0)
        assert np.array_equal(hs._indices, h0._indices[h0._indptr[s0]:]) and np.array_equal(hs._indptr, h0._indptr[s0:] - h0._indptr[s0])
        assert np.array_equal(ts._values, t0._values[t0._indptr[s0]:])


def test_ranges_and_folds(hiplib):
    import ppca_rs_amd as P

    x, w, _ = SC.case(257, 300, 1)
    sp = P.SparseDataset.from_dense(x, w)
    a, b = sp.holdout(0.35, 9), sp.holdout_range(0.0, 0.35, 9)
    for p, q in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(p.csr(), q.csr())) and p.holdout_counts == q.holdout_counts
    assert P.SparseDataset.fold_edges(4) == P.Dataset.fold_edges(4) == [0.0, 0.25, 0.5, 0.75, 1.0]
    for nf in (2, 3, 7):
        parts = sp.kfold(nf, 9)
        assert len(parts) == nf
        times = np.zeros(sp.nnz, dtype=int)
        for train, held in parts:
            _check_parts(sp, train, held)
            times += np.isin(_positions(sp), _positions(held))
        assert np.all(times == 1)  # every entry is held in exactly one fold
        assert sum(h.nnz for _, h in parts) == sp.nnz
    # one fresh seed serves every fold of a call
    parts = sp.kfold(3)
    assert sum(h.nnz for _, h in parts) == sp.nnz
    assert len(np.unique(np.concatenate([_positions(h) for _, h in parts]))) == sp.nnz


def test_bad_arguments(hiplib):
    import ppca_rs_amd as P

    x, _, _ = SC.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x)
    for f in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            sp.holdout(f, 1)
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.5, 1.5), (float("nan"), 0.5), (0.2, float("nan"))):
        with pytest.raises(ValueError):
            sp.holdout_range(lo, hi, 1)
    with pytest.raises(ValueError):
        sp.holdout(0.1, 1, row_offset=-1)
    with pytest.raises(ValueError):
        sp.holdout_range(0.1, 0.2, 1, row_offset=-1)
    for nf in (1, 0):
        with pytest.raises(ValueError):
            sp.kfold(nf, 1)
    # the routine itself
    indptr, indices, _ = sp.csr()
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.5, 1.5), (float("nan"), 0.5), (0.2, float("nan")), (1.5, 1.5)):
        rc, _, _ = _split(hiplib, indptr, indices, lo, hi, 1, 0)
        assert rc == INVALID and hiplib.ppca_last_error(), (lo, hi)
    assert _split(hiplib, indptr, indices, 0.0, 0.5, 1, -1)[0] == INVALID
    bad = indptr.copy()
    bad[3], bad[4] = bad[4] + 1, bad[3]
    assert _split(hiplib, bad, indices, 0.0, 0.5, 1, 0)[0] == INVALID  # non-monotone row_ptr
    assert _split(hiplib, indptr, indices, 0.0, 0.5, 1, 0)[0] == 0
    # no rows: nothing to flag
    rc, flags, counts = _split(hiplib, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 0.0, 0.5, 1, 0)
    assert rc == 0 and tuple(counts) == (0, 0)
    e0, e1 = P.SparseDataset([0], [], [], 3).holdout(0.5, 1)
    assert len(e0) == len(e1) == 0 and e0.holdout_counts == (0, 0)


def test_a_fresh_seed_per_call(hiplib):
    import ppca_rs_amd as P

    x, _, _ = SC.case(257, 300, 1)
    sp = P.SparseDataset.from_dense(x)
    a, b = sp.holdout(0.5), sp.holdout(0.5)
    assert sum(a[0].holdout_counts) == sum(b[0].holdout_counts) == sp.nnz
    assert not np.array_equal(_positions(a[1]), _positions(b[1]))


def test_what_stays_dense_only_says_so(hiplib):
    import ppca_rs_amd as P

    x, _, (s, c, mu) = SC.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x)
    train, held = sp.holdout(0.3, 1)
    model = P.PPCAModel(s, c, mu)
    with pytest.raises(TypeError):
        model.heldout_score(train, P.Dataset.__new__(P.Dataset))  # one of each
    with pytest.raises(ValueError):
        model.heldout_score(train, P.SparseDataset.from_dense(x[:-1]))
    with pytest.raises(ValueError, match="block_rows"):
        model.heldout_score(train, P.SparseDataset.from_dense(x, block_rows=16))
    with pytest.raises(TypeError):
        P.heldout_score(P.FAModel(np.ones(9), c, mu), train, held)
    with pytest.raises(ValueError, match="precisions"):
        P.cross_validate(sp, lambda tr: model, folds=3, seed=1, precisions=np.ones((64, 9)))
    with pytest.raises(ValueError, match="pca"):
        P.PPCATrainer(sp).select_state_size([2], fraction=0.2, seed=1, init="pca")


# ------------------------------------------------------------------ the C-ABI
def test_abi_has_the_new_symbols(hiplib):
    import test_abi
    from ppca_rs_amd import _lib

    for name in ("ppca_heldout_split_csr_host", "ppca_heldout_score_sparse"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES and name in test_abi._declared_symbols()
