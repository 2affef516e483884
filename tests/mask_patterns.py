"""STRUCTURED missing-data patterns for the oracle comparisons (tests/test_mask_patterns_host.py, tests/test_gpu_mask_patterns.py).  No
test lives here.

Every other GPU test masks i.i.d. Bernoulli (oracle.synth), under which every mask word of every row is a random mix of bits.  The
kernels read the mask in bit-level ways that such data never stresses:

  * the fused kernels keep a row's mask as four u64 words -- word 2h + e, bit l stands for dimension 128 h + 2 l + e -- and count by
    popcount: `words`, `checker`, `checker2`, `edges`, `stripe64`, `staircase` make words that are all zero, all ones, one bit at either
    end or at the 31/32 split, or only the ragged tail past d;
  * the fixed-point statistics take their column exponents from the workgroup's FIRST tile and contract two 32-row tiles per int8
    MFMA: `tile_blocks` and `thin_tiles` give empty first tiles, empty 64-row groups and half groups, and tiles with a handful of live
    rows under the floor exponent; the split pipeline predicts a chunk's digit scales from the chunk before (an empty chunk);
  * rows with fewer observed entries than the state size leave C_o^T C_o rank-deficient, so the solve rests on sigma^2 I: `single`,
    `rank_edge`, `sparse97`; columns seen in one row or none: `column_once`.

True = observed; i is the row, j the column."""
import numpy as np

NAMES = ("full", "single", "rank_edge", "words", "stripe64", "edges", "tile_blocks", "thin_tiles", "staircase", "column_once",
         "checker", "checker2", "sparse97")
EDGE_COLUMNS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 254, 255)
TILE = 32
EMPTY_TILE_ROWS = ((0, 32), (64, 128), (160, 192))  # `tile_blocks`, besides the last partial tile
THIN_BELOW, THIN_EVERY = 160, 11  # `thin_tiles`: below row 160 only every 11th row lives, none in the first tile


def once_columns(d):
    """`column_once`: the columns observed in exactly one row (column 1 in none)"""
    return (3 % d, d // 2, d - 1)


def once_rows(n):
    """... and the row of each"""
    return (5, n // 2, n - 2)


def edge_columns(d):
    return sorted({c for c in EDGE_COLUMNS + (d - 2, d - 1) if 0 <= c < d})


def last_partial_tile(n):
    """(first row, n) of the tile that n leaves incomplete; (n, n) if there is none"""
    return (n - n % TILE, n)


def patterns(n, d, k, seed):
    """name -> bool (n, d), in the order of NAMES; deterministic in (n, d, k, seed)."""
    rng = np.random.default_rng(seed)
    i, j = np.arange(n)[:, None], np.arange(d)[None, :]
    out = {}
    out["full"] = np.ones((n, d), dtype=bool)
    out["single"] = j == i % d
    m = np.zeros((n, d), dtype=bool)
    for r in range(n):  # 0 .. k + 2 observed entries: below, at and above the state size, and all-masked rows
        m[r, rng.permutation(d)[:min(r % (k + 3), d)]] = True
    out["rank_edge"] = m
    out["words"] = (j // 128) * 2 + j % 2 == i % 4
    out["stripe64"] = j // 64 == i % -(-d // 64)
    m = np.zeros((n, d), dtype=bool)
    cols = edge_columns(d)
    m[:, cols] = rng.random((n, len(cols))) < 0.7
    out["edges"] = m
    m = rng.random((n, d)) < 0.7
    for a, b in EMPTY_TILE_ROWS + (last_partial_tile(n),):
        m[a:b] = False
    out["tile_blocks"] = m
    m = rng.random((n, d)) < 0.7
    rows = np.arange(n)
    m[(rows < THIN_BELOW) & (rows % THIN_EVERY != 0)] = False
    m[:TILE] = False
    out["thin_tiles"] = m
    out["staircase"] = j < 1 + (i * d) // n
    m = rng.random((n, d)) < 0.7
    m[:, 1] = False
    for col, row in zip(once_columns(d), once_rows(n)):
        m[:, col] = False
        m[row, col] = True
    out["column_once"] = m
    out["checker"] = (i + j) % 2 == 0
    out["checker2"] = (i + j // 2) % 2 == 0
    out["sparse97"] = rng.random((n, d)) < 0.03
    assert tuple(out) == NAMES
    return out


def mask_words(mask):
    """(n, 4) uint64: the fused kernels' four mask words of every row (word 2h + e, bit l <-> dimension 128 h + 2 l + e), d <= 256."""
    n, d = mask.shape
    assert d <= 256
    words = np.zeros((n, 4), dtype=np.uint64)
    for col in range(d):
        h, l, e = col // 128, (col % 128) // 2, col % 2
        words[:, 2 * h + e] |= mask[:, col].astype(np.uint64) << np.uint64(l)
    return words


def case(oracle, n, d, k, name, seed):
    """(x, w, (s, c, mu), mask): the values of oracle.synth(n, d, k, 0.0, seed) under pattern `name`; the model and the weights as in
    tests/test_gpu_split_steady_state.py::_case.  Read-only: callers share it."""
    rng = np.random.default_rng(seed)
    x, _, _ = oracle.synth(n, d, k, 0.0, seed)
    mask = patterns(n, d, k, seed)[name]
    x[~mask] = np.nan
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.7
    w = rng.uniform(0.25, 2.0, n)
    for a in (x, w, c, mu, mask):
        a.setflags(write=False)
    return x, w, (s, c, mu), mask
