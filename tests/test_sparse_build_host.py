"""CPU-only: the device-side build of SparseDataset as far as it can be held without a GPU -- the four new C-ABI
symbols, the argument checks of SparseDataset.from_device (before the library is touched), `on_device=None` on a host-born dataset
(today's host split, no context), and the numpy restatement of the container (tests/sparse_build_cases.py), the second oracle of
tests/test_gpu_sparse_build.py, against ppca_sparse_transpose_host on every case and tiling."""
import ctypes as C

import numpy as np
import pytest

import sparse_build_cases as B

NEW_SYMBOLS = ("ppca_from_device_sparse", "ppca_index_to_host_sparse", "ppca_n_blocks_sparse", "ppca_heldout_split_sparse")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_library_exports_the_new_symbols(hiplib):
    from ppca_rs_amd import _lib

    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(hiplib, name) is not None, name


def test_from_device_checks_its_arguments_before_the_library(hiplib, monkeypatch):
    import ppca_rs_amd as P
    from ppca_rs_amd import api

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(api, "lib", touched)
    monkeypatch.setattr(api, "_ctx", touched)
    good = dict(indptr_ptr=4096, indices_ptr=8192, values_ptr=12288, n=3, n_columns=5)
    for bad in (dict(indptr_ptr=0), dict(indptr_ptr=None), dict(n=-1), dict(n_columns=0), dict(n_columns=2 ** 31), dict(block_rows=0),
                dict(segment=-2)):
        with pytest.raises(ValueError):
            P.SparseDataset.from_device(**{**good, **bad})
    with pytest.raises(AssertionError, match="touched"):  # (the good arguments do reach it)
        P.SparseDataset.from_device(**good)


@pytest.mark.parametrize("name", ["seams", "wide"])
def test_on_device_none_is_the_host_split_on_a_host_born_dataset(hiplib, name):
    import ppca_rs_amd as P
    from ppca_rs_amd import _lib

    indptr, indices, values, d = B.case(name)
    before = _lib._default_ctx
    sp = P.SparseDataset(indptr, indices, values, d, B.weights_of(name), block_rows=64, segment=8)
    flags, counts = np.zeros(indices.size, dtype=np.uint8), np.zeros(2, dtype=np.int64)
    assert hiplib.ppca_heldout_split_csr_host(len(sp), _ptr(indptr), _ptr(indices), 0.0, 0.3, 11, 5, _ptr(flags), _ptr(counts)) == 0
    held = flags.view(np.bool_)
    for train, heldp in (sp.holdout(0.3, 11, row_offset=5), sp.holdout(0.3, 11, row_offset=5, on_device=None),
                         sp.holdout_range(0.0, 0.3, 11, row_offset=5, on_device=False)):
        for part, keep in ((train, ~held), (heldp, held)):
            ip, ix, v = part.csr()
            assert np.array_equal(ip, np.concatenate([[0], np.cumsum(keep)])[indptr]) and np.array_equal(ix, indices[keep])
            assert np.array_equal(v.view(np.uint64), values[keep].view(np.uint64))
            assert part.holdout_counts == (int(counts[0]), int(counts[1])) and np.array_equal(part.weights(), B.weights_of(name))
            assert part._handle is None and part._ctx_arg is None
    folds = sp.kfold(3, 11, on_device=None)
    assert sum(h.nnz for _, h in folds) == sp.nnz and all(t._handle is None and h._handle is None for t, h in folds)
    assert sp._handle is None and sp._ctx_arg is None and _lib._default_ctx is before  # no context was made, no device touched


def _transpose(hiplib, indptr, indices, values, d, block_rows):
    n, nnz = len(indptr) - 1, indices.size
    br = B.tiling_of(block_rows, None)[0]
    nb = -(-n // br)
    cp = np.full((max(nb, 1), d + 1), -1, dtype=np.int64)
    tr, tv = np.full(max(nnz, 1), -1, dtype=np.int32), np.full(max(nnz, 1), np.nan)
    assert hiplib.ppca_sparse_transpose_host(n, d, _ptr(indptr), _ptr(indices), _ptr(values), block_rows or 0, _ptr(cp), _ptr(tr), _ptr(tv)) == 0
    return cp[:nb], tr[:nnz], tv[:nnz]


@pytest.mark.parametrize("tiling", B.TILINGS, ids=B.TILING_IDS)
@pytest.mark.parametrize("name", B.NAMES)
def test_the_restatement_against_the_host_transpose(hiplib, name, tiling):
    indptr, indices, values, d = B.case(name)
    blocks = B.restate(indptr, indices, values, d, *tiling)
    cp, tr, tv = _transpose(hiplib, indptr, indices, values, d, tiling[0])
    br, seg = B.tiling_of(*tiling)
    assert len(blocks) == len(cp) == -(-(len(indptr) - 1) // br)
    for i, b in enumerate(blocks):
        c = b["counts"]
        e0, e1 = c["e0"], c["e0"] + c["nnz"]
        assert (c["row0"], e0, e1) == (i * br, indptr[i * br], indptr[i * br + c["rows"]])
        assert np.array_equal(b["col_ptr"], cp[i]) and np.array_equal(b["t_row"], tr[e0:e1])
        assert np.array_equal(b["t_val"].view(np.uint64), tv[e0:e1].view(np.uint64))
        # the row lists: a partition of the block's rows by length, each bin ascending
        lengths = np.diff(indptr[c["row0"]:c["row0"] + c["rows"] + 1])
        assert sorted(b["rowlist"].tolist()) == list(range(c["rows"])) and c["nbin0"] + c["nbin1"] + c["nbin2"] == c["rows"]
        for k, (lo, hi) in enumerate(((-1, B.SHORT), (B.SHORT, B.MID), (B.MID, d))):
            part = b["rowlist"][c["off%d" % k]:c["off%d" % k] + c["nbin%d" % k]]
            assert np.all(np.diff(part) > 0) and np.all((lengths[part] > lo) & (lengths[part] <= hi))
        # the items: every column's entries exactly once, in column order, runs of seg with a shorter last one
        it, lg = b["items"], b["longs"]
        assert c["n_items"] == len(it) and c["n_long"] == len(lg) and c["n_runs"] == int(lg["nruns"].sum())
        assert np.array_equal(np.bincount(it["col"], weights=it["len"], minlength=d).astype(np.int64), np.diff(cp[i]))
        assert np.all(np.diff(it["start"]) == it["len"][:-1]) and np.all((it["len"] >= 1) & (it["len"] <= seg))
        if len(it):
            assert it["start"][0] == e0 and it["start"][-1] + it["len"][-1] == e1
        runs = it[it["dest"] >= 0]
        assert np.array_equal(runs["dest"], np.arange(c["n_runs"])) and np.all(it["dest"] >= -1)
        assert np.array_equal(lg["first"], np.concatenate([[0], np.cumsum(lg["nruns"])[:-1]])[:len(lg)])
        assert np.array_equal(lg["col"], np.flatnonzero(np.diff(cp[i]) > seg))
