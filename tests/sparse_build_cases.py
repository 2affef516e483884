"""Inputs of the device-side build of SparseDataset (tests/test_sparse_build_host.py and
tests/test_gpu_sparse_build.py) and a numpy restatement of the container, written from the comment at the head of
ppca_rs_amd/csrc/ppca_sparse.hpp: the three row lists by row length, the inverted index in CSC order, the work items and long columns.

CASES: name -> (indptr int64, indices int32, values float64, n_columns), built once and read-only.
  seams   (300, 300), meant for block_rows = 64, segment = 8: rows of 0, 1, 15, 16, 17, 63, 64, 65 and d entries (block 0); columns with
          0, 1, 7, 8, 9, 16 and 17 = 2 segment + 1 entries in a block (block 1); an empty block (2); a ragged last block (44 rows); an
          empty first and last row
  one     (1, 1) with its one entry;  nnz0  five rows without an entry;  d1  one column
  wide    (40, 70 000), row 0 full but for one column: columns above 2^16, a third radix digit
  big     (400, 1000) at 30 %: one block of about 120 000 entries under the default tiling, every value of the low digit in use
TILINGS: (block_rows, segment), None = the library's default."""
import functools

import numpy as np

import sparse_cases as SC

SHORT, MID = 16, 64                                         # row-length bins: m <= 16, m <= 64, longer
DEFAULT_BLOCK_ROWS = (1 << 30) // (8 * (16 + 1 + 16 * 17 // 2))  # the records of a block stay under 1 GiB at k = 16
DEFAULT_SEGMENT = 512
SEAMS_TILING = (64, 8)
TILINGS = [SEAMS_TILING, (64, None), (None, 8), (7, 3)]
TILING_IDS = ["b%s-s%s" % t for t in TILINGS]
NAMES = ["seams", "one", "nnz0", "d1", "wide", "big"]
ITEM = np.dtype([("start", "<i8"), ("dest", "<i8"), ("col", "<i4"), ("len", "<i4")])
LONG = np.dtype([("first", "<i8"), ("col", "<i4"), ("nruns", "<i4")])
COUNTS = ("row0", "rows", "e0", "nnz", "nbin0", "nbin1", "nbin2", "off0", "off1", "off2", "n_items", "n_long", "n_runs")


def _csr(obs, rng):
    indptr = np.concatenate([[0], np.cumsum(obs.sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(obs)[1].astype(np.int32)
    return indptr, indices, rng.standard_normal(indices.size)


def _seams(rng):
    n = d = 300
    obs = np.zeros((n, d), dtype=bool)
    for i, m in zip(range(1, 10), (1, 15, 16, 17, 63, 64, 65, d, 0)):  # block 0; row 0 stays empty
        obs[i, rng.choice(d, size=m, replace=False)] = True
    for j, cnt in zip(range(10, 16), (1, 7, 8, 9, 16, 17)):  # block 1: column j has exactly cnt entries, every other column none
        obs[64 + rng.choice(64, size=cnt, replace=False), j] = True
    # block 2 (rows 128 .. 191) has no entry
    obs[192:256] = rng.random((64, d)) < 0.10
    obs[256:299] = rng.random((43, d)) < 0.25  # the ragged block; row 299 stays empty
    return _csr(obs, rng) + (d,)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(4310 + NAMES.index(name))
    if name == "seams":
        out = _seams(rng)
    elif name == "one":
        out = (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([1.5]), 1)
    elif name == "nnz0":
        out = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), 4)
    elif name == "d1":
        out = _csr(rng.random((9, 1)) < 0.6, rng) + (1,)
    elif name == "wide":
        x, _, _ = SC.case(40, 70000, 3)
        out = SC.csr_of(x) + (70000,)
        assert out[1].max() > 65535
    elif name == "big":
        out = _csr(rng.random((400, 1000)) < 0.30, rng) + (1000,)
        assert 110_000 < out[1].size < 130_000 and np.unique(out[1] & 255).size == 256
    else:
        raise KeyError(name)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def weights_of(name):
    n = len(case(name)[0]) - 1
    w = 0.5 + np.random.default_rng(99).random(n)
    w.setflags(write=False)
    return w


def tiling_of(block_rows, segment):
    return block_rows or DEFAULT_BLOCK_ROWS, segment or DEFAULT_SEGMENT


def restate(indptr, indices, values, d, block_rows=None, segment=None):
    """The container as the header comment defines it: a list, per block of block_rows rows, of dicts with `counts` (COUNTS), `col_ptr`
    (d + 1, relative to the block's first entry), `t_row`, `t_val`, `rowlist`, `items` (ITEM) and `longs` (LONG)."""
    br, seg = tiling_of(block_rows, segment)
    n = len(indptr) - 1
    out = []
    for row0 in range(0, n, br):
        rows = min(n, row0 + br) - row0
        e0, e1 = int(indptr[row0]), int(indptr[row0 + rows])
        lengths = np.diff(indptr[row0:row0 + rows + 1])
        local = np.arange(rows, dtype=np.int32)
        bins = [local[lengths <= SHORT], local[(lengths > SHORT) & (lengths <= MID)], local[lengths > MID]]  # each in ascending row
        col = indices[e0:e1]
        order = np.argsort(col, kind="stable")  # per column, the block's entries in ascending row
        t_row = np.repeat(local, lengths)[order].astype(np.int32)
        t_val = values[e0:e1][order]
        cnt = np.bincount(col, minlength=d)
        col_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        items, longs, n_runs = [], [], 0
        for j in np.flatnonzero(cnt):
            c = int(cnt[j])
            if c <= seg:  # one item that adds into the statistics
                items.append((e0 + col_ptr[j], -1, j, c))
            else:  # runs of exactly seg entries, the last one shorter, each an item that writes a partial
                nruns = -(-c // seg)
                longs.append((n_runs, j, nruns))
                for r in range(nruns):
                    items.append((e0 + col_ptr[j] + r * seg, n_runs + r, j, min(seg, c - r * seg)))
                n_runs += nruns
        nb = [len(b) for b in bins]
        counts = dict(zip(COUNTS, [row0, rows, e0, e1 - e0] + nb + [0, nb[0], nb[0] + nb[1]] + [len(items), len(longs), n_runs]))
        out.append(dict(counts=counts, col_ptr=col_ptr, t_row=t_row, t_val=t_val, rowlist=np.concatenate(bins).astype(np.int32),
                        items=np.array(items, dtype=ITEM), longs=np.array(longs, dtype=LONG)))
    return out


def same_index(a, b):
    """The names of what differs between two block lists (restate's form); values compare as bits."""
    if len(a) != len(b):
        return ["n_blocks %d != %d" % (len(a), len(b))]
    bad = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x["counts"] != y["counts"]:
            bad.append("block %d counts %s != %s" % (i, x["counts"], y["counts"]))
        for key in ("col_ptr", "t_row", "rowlist"):
            if key in x and key in y and not np.array_equal(x[key], y[key]):
                bad.append("block %d %s" % (i, key))
        if not np.array_equal(x["t_val"].view(np.uint64), y["t_val"].view(np.uint64)):
            bad.append("block %d t_val" % i)
        for key, dt in (("items", ITEM), ("longs", LONG)):
            for f in dt.names:
                if not np.array_equal(x[key][f], y[key][f]):
                    bad.append("block %d %s.%s" % (i, key, f))
    return bad
