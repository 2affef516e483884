"""tests/mask_patterns.py on the host: every pattern keeps the property it is named for, the generator is deterministic, and on every
pattern the two CPU restatements of the reference -- oracle/ppca_oracle.c and the independent literal port oracle/restate_numpy.py --
agree to 1e-10 relative (measured: <= 3e-12), so that what tests/test_gpu_mask_patterns.py measures at 1e-9 .. 1e-7 is the kernels and not
the reference.  No GPU."""
import numpy as np
import pytest

import mask_patterns as MP

N = 293
DS = (64, 70, 200, 256, 300)
K = 4
ORACLE_SHAPES = ((70, 4), (200, 7))
ORACLE_BOUND = 1e-10


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module", params=DS)
def pats(request):
    d = request.param
    return d, MP.patterns(N, d, K, 17 + d)


def test_names_shapes_and_types(pats):
    d, p = pats
    assert tuple(p) == MP.NAMES and len(MP.NAMES) == 13
    for name, m in p.items():
        assert m.shape == (N, d) and m.dtype == np.bool_, name


def test_full_and_single(pats):
    d, p = pats
    assert p["full"].all()
    assert (p["single"].sum(1) == 1).all()
    assert (p["single"].argmax(1) == np.arange(N) % d).all()


def test_rank_edge_counts_straddle_the_state_size(pats):
    d, p = pats
    counts = p["rank_edge"].sum(1)
    assert (counts == np.arange(N) % (K + 3)).all()
    assert {0, 1, K - 1, K, K + 1} <= set(counts.tolist())
    assert len({tuple(np.flatnonzero(r)) for r in p["rank_edge"][counts == K]}) > 1  # (chosen at random, not one fixed set)


def _word_of(d):
    j = np.arange(d)
    return (j // 128) * 2 + j % 2


def test_words_one_word_per_live_row(pats):
    d, p = pats
    word = _word_of(d)
    m = p["words"]
    for i in range(N):
        if (word == i % 4).any():
            assert set(word[m[i]].tolist()) == {i % 4} and m[i][word == i % 4].all(), i
        else:
            assert not m[i].any(), i  # (d <= 128: words 2 and 3 have no dimension)
    if d <= 256:
        w = MP.mask_words(m)
        live = m.any(1)
        assert ((w != 0).sum(1)[live] == 1).all() and (w[~live] == 0).all()
        if d == 256:
            assert (w[np.arange(N), np.arange(N) % 4] == np.uint64(2 ** 64 - 1)).all()


def test_stripe64_and_its_ragged_tail(pats):
    d, p = pats
    nb = -(-d // 64)
    m = p["stripe64"]
    for i in range(N):
        b = i % nb
        want = np.zeros(d, dtype=bool)
        want[64 * b:min(64 * b + 64, d)] = True
        assert np.array_equal(m[i], want), i
    assert m[nb - 1].sum() == d - 64 * (nb - 1)


def test_edges_only_the_word_boundaries(pats):
    d, p = pats
    cols = [c for c in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 254, 255, d - 2, d - 1) if c < d]
    m = p["edges"]
    other = np.ones(d, dtype=bool)
    other[cols] = False
    assert not m[:, other].any()
    frac = m[:, cols].mean(0)
    assert (frac > 0.55).all() and (frac < 0.85).all()  # 0.7 +- 5.6 sigma at n = 293
    assert {d - 2, d - 1} <= set(MP.edge_columns(d)) and MP.edge_columns(d) == sorted(set(cols))


def test_tile_blocks_empty_and_live_ranges(pats):
    d, p = pats
    live = p["tile_blocks"].any(1)
    for a, b in ((0, 32), (64, 128), (160, 192), (288, 293)):
        assert not live[a:b].any(), (a, b)
    for a, b in ((32, 64), (128, 160), (192, 288)):
        assert live[a:b].all(), (a, b)
    assert MP.last_partial_tile(N) == (288, 293) and MP.last_partial_tile(64) == (64, 64)
    frac = p["tile_blocks"][live].mean()
    assert 0.67 < frac < 0.73


def test_thin_tiles_few_live_rows_under_an_empty_first_tile(pats):
    d, p = pats
    live = p["thin_tiles"].any(1)
    rows = np.arange(N)
    assert not live[:32].any()
    assert np.array_equal(live[32:160], rows[32:160] % 11 == 0)
    assert live[160:].all()
    per_tile = [int(live[a:a + 32].sum()) for a in range(0, 160, 32)]
    assert per_tile[0] == 0 and all(1 <= c <= 8 for c in per_tile[1:]), per_tile  # (at most the eight rows that may go round the fixed-point form)


def test_staircase_is_a_monotone_prefix(pats):
    d, p = pats
    m = p["staircase"]
    counts = m.sum(1)
    assert (counts == 1 + (np.arange(N) * d) // N).all() and counts[0] == 1 and counts[-1] == min(d, 1 + ((N - 1) * d) // N)
    assert (np.diff(counts) >= 0).all()
    for i in range(N):
        assert m[i, :counts[i]].all()


def test_column_once(pats):
    d, p = pats
    m = p["column_once"]
    assert m[:, 1].sum() == 0
    for col, row in zip((3 % d, d // 2, d - 1), (5, N // 2, N - 2)):
        assert m[:, col].sum() == 1 and m[row, col], (col, row)
    rest = np.ones(d, dtype=bool)
    rest[[1, 3 % d, d // 2, d - 1]] = False
    assert (m[:, rest].sum(0) > 150).all()


def test_checkers_as_mask_words():
    ones, fives, aaaa = np.uint64(2 ** 64 - 1), np.uint64(0x5555555555555555), np.uint64(0xAAAAAAAAAAAAAAAA)
    p = MP.patterns(N, 256, K, 1)
    w = MP.mask_words(p["checker"])
    assert (w[0::2] == np.array([ones, 0, ones, 0], dtype=np.uint64)).all() and (w[1::2] == np.array([0, ones, 0, ones], dtype=np.uint64)).all()
    w = MP.mask_words(p["checker2"])
    assert (w[0::2] == fives).all() and (w[1::2] == aaaa).all()
    for d in DS:
        p = MP.patterns(N, d, K, 1)
        i, j = np.indices((N, d))
        assert np.array_equal(p["checker"], (i + j) % 2 == 0) and np.array_equal(p["checker2"], (i + j // 2) % 2 == 0)


def test_mask_words_layout():
    m = np.zeros((6, 256), dtype=bool)
    for r, col in enumerate((0, 1, 127, 128, 254, 255)):
        m[r, col] = True
    w = MP.mask_words(m)
    want = [(0, 0), (1, 0), (1, 63), (2, 0), (2, 63), (3, 63)]
    for r, (word, bit) in enumerate(want):
        assert w[r, word] == np.uint64(1) << np.uint64(bit) and (w[r] != 0).sum() == 1, r


def test_sparse97_density(pats):
    d, p = pats
    frac = p["sparse97"].mean()
    assert 0.02 < frac < 0.04  # 0.03 +- 8 sigma at the smallest shape
    assert not p["sparse97"].all(1).any()


def test_deterministic_in_the_seed():
    a, b, c = MP.patterns(N, 70, K, 5), MP.patterns(N, 70, K, 5), MP.patterns(N, 70, K, 6)
    for name in MP.NAMES:
        assert np.array_equal(a[name], b[name]), name
    for name in ("rank_edge", "edges", "tile_blocks", "thin_tiles", "column_once", "sparse97"):
        assert not np.array_equal(a[name], c[name]), name


def test_case_masks_the_synthetic_values(oracle):
    x, w, (s, c, mu), mask = MP.case(oracle, N, 70, K, "tile_blocks", 3)
    full, _, _ = oracle.synth(N, 70, K, 0.0, 3)
    assert np.array_equal(np.isfinite(x), mask) and np.array_equal(x[mask], full[mask])
    assert c.shape == (70, K) and mu.shape == (70,) and s == 0.7 and w.shape == (N,) and w.min() >= 0.25 and w.max() <= 2.0
    x2, w2, (_, c2, mu2), _ = MP.case(oracle, N, 70, K, "tile_blocks", 3)
    assert np.array_equal(x, x2, equal_nan=True) and np.array_equal(w, w2) and np.array_equal(c, c2) and np.array_equal(mu, mu2)
    assert not x.flags.writeable


@pytest.mark.parametrize("name", MP.NAMES)
@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=lambda s: "d%d-k%d" % s)
def test_the_two_cpu_restatements_agree(oracle, shape, name):
    """llks, states, covariances and one weighted EM step of oracle/ppca_oracle.c against oracle/restate_numpy.py."""
    from oracle import restate_numpy as R

    d, k = shape
    x, w, (s, c, mu), _ = MP.case(oracle, N, d, k, name, 40 + d)
    errs = {"llks": _rel(oracle.llks(x, s, c, mu), R.llks(x, s, c, mu))}
    st, cv = oracle.infer(x, s, c, mu)
    ref = [R.infer_one(s, c, mu, row) for row in x]
    errs["states"] = _rel(st, np.array([r[0] for r in ref]))
    errs["covariances"] = _rel(cv, np.array([r[1] for r in ref]))
    s1, c1, m1 = oracle.iterate(x, s, c, mu, w)
    s2, c2, m2 = R.iterate_with_prior(x, s, c, mu, w)
    errs["sigma"], errs["C"], errs["mean"] = abs(s1 - s2) / s2, _rel(c1, c2), _rel(m1, m2)
    print(name, shape, " ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) < ORACLE_BOUND, errs
