"""The fused EM pass at the shapes where the address arithmetic of its front role's memory requests can go wrong.  The order in
which the front waves queue those requests (digit-table loads spread through the b loop) changes nothing that is computed, so
every case is the pass against the CPU oracle: the raw statistics block by block at 1e-9 (as test_stats_raw_against_oracle) and
two EM steps at RTOL.

Shapes: workgroups that walk exactly 0, 1, 2, 3 and all tiles (grid limits 1, 3 and 4 at n = 200 = 6 tiles + 8 rows and
n = 5 * 32 + 7; the full grid at n = 1 000: one tile per workgroup), a last tile of 1 and of 31 rows, d = 256 / 200 / 7 / 5 (row
pitches that are and are not multiples of the 128-byte line), k = 1 / 4 / 10, weights, a column slice of a wider host array, a row
slice of a larger device dataset that ends at the parent's last row, and the mixture's gathered weighted pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # north_star tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _check_pass(P, oracle, ds, x, w, d, k, seed, tag):
    """ds holds the rows x (weights w or None): raw statistics and two EM steps against the oracle."""
    from ppca_rs_amd import _lib

    x = np.ascontiguousarray(x)
    rng = np.random.default_rng(seed)
    c, mu, s = rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d), 0.7
    m = P.PPCAModel(s, c, mu)
    n = _lib.lib().ppca_stats_len(d, k)
    got = np.empty(n)
    _lib.check(_lib.lib().ppca_stats_raw(ds._ctx.handle, ds._h, m._device(ds._ctx).h, _lib.ptr(got)))
    want = oracle.stats(x, s, c, mu, w)
    kp = k * (k + 1) // 2
    bounds = [0, d * k, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d, 2 * d * k + d * kp + 2 * d, n]
    for name, a, b in zip(["cross", "S", "U", "sumx", "totals", "scalars"], bounds[:-1], bounds[1:]):
        assert _rel(got[a:b], want[a:b]) < 1e-9, (tag, name)
    for it in range(2):
        want_llk = oracle.llk(x, s, c, mu, w)
        s, c, mu = oracle.iterate(x, s, c, mu, w)
        m, llk = m.iterate_with_llk(ds)
        assert abs(llk - want_llk) < RTOL * abs(want_llk), (tag, it)
        assert abs(m.isotropic_noise - s) < RTOL * s, (tag, it)
        assert _rel(m.transform, c) < RTOL, (tag, it)
        assert _rel(m.mean, mu) < RTOL, (tag, it)


def _data(oracle, n, d, k, seed):
    x, _, _ = oracle.synth(n, d, k, 0.3, seed)
    if n > 10:
        x[10] = np.nan  # an all-masked row
    return x


# (n, d, k, grid limit, weighted)
CASES = [
    (200, 256, 10, 1, False),   # one workgroup walks all seven tiles, the last of 8 rows
    (200, 256, 10, 3, False),   # workgroups of 3, 3 and 1 tiles
    (167, 256, 10, 1, False),   # six tiles, the last of 7 rows
    (167, 256, 10, 3, False),   # workgroups of 2 tiles each
    (167, 200, 4, 4, False),    # 2, 2, 2 and 0 tiles
    (1000, 256, 10, 0, False),  # the full grid: one tile or none per workgroup, a last tile of 8 rows
    (1000, 200, 10, 0, False),
    (65, 7, 1, 0, False),       # a last tile of one row
    (65, 256, 10, 1, False),
    (95, 5, 4, 1, False),       # a last tile of 31 rows
    (95, 256, 4, 3, False),
    (200, 5, 1, 3, False),
    (200, 7, 4, 1, False),
    (200, 200, 1, 1, False),
    (200, 256, 10, 1, True),
    (167, 7, 1, 3, True),
    (1000, 200, 4, 0, True),
]


@pytest.mark.parametrize("n,d,k,limit,weighted", CASES, ids=["n%d-d%d-k%d-g%d%s" % (c[0], c[1], c[2], c[3], "-w" if c[4] else "") for c in CASES])
def test_pass_against_oracle(P, oracle, n, d, k, limit, weighted):
    from ppca_rs_amd import _lib

    x = _data(oracle, n, d, k, 7000 + n + d + k)
    w = np.random.default_rng(n + d).uniform(0.5, 1.5, n) if weighted else None
    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(limit)
        _check_pass(P, oracle, P.Dataset(x, w), x, w, d, k, 31 * d + k, (n, d, k, limit, weighted))
    finally:
        ctx.set_grid_limit(0)


@pytest.mark.parametrize("limit", [0, 1, 3])
def test_column_slice_of_a_wider_array(P, oracle, limit):
    """A 100-column view of a 256-column host array: the host's row stride is not the dataset's row length."""
    from ppca_rs_amd import _lib

    n, d, k = 200, 100, 4
    wide = np.full((n, 256), 1e300)  # (what lies beside the view must never be read as data)
    view = wide[:, 50:150]
    view[...] = _data(oracle, n, d, k, 811)
    assert view.strides[0] == 256 * 8 and not view.flags["C_CONTIGUOUS"]
    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(limit)
        _check_pass(P, oracle, P.Dataset(view), view, None, d, k, 5, ("view", limit))
    finally:
        ctx.set_grid_limit(0)


@pytest.mark.parametrize("d,k,limit", [(256, 10, 1), (256, 10, 3), (200, 4, 0), (7, 4, 1)])
def test_row_slice_ending_at_the_parents_last_row(P, oracle, d, k, limit):
    """The rows [133, 300) of a 300-row device dataset: the slice's last tile (7 rows) ends where the parent's allocation ends, so a
    request past the slice's rows would leave the allocation."""
    from ppca_rs_amd import _lib

    n, start = 300, 133
    x = _data(oracle, n, d, k, 900 + d)
    parent = P.Dataset(x)
    sub = parent._slice(start, n - start)
    assert len(sub) == n - start
    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(limit)
        _check_pass(P, oracle, sub, x[start:], None, d, k, 17 + d, ("slice", d, k, limit))
    finally:
        ctx.set_grid_limit(0)


def test_mixture_gathered_pass(P, oracle):
    """Two PPCAMix.iterate steps at d = 16, k = 3, K = 2: every component's statistics come from the gathered, weighted
    instantiation of the pass."""
    rng = np.random.default_rng(9)
    d, k, nm, n = 16, 3, 2, 1000
    x = np.concatenate([oracle.synth(n // nm, d, k, 0.25, 300 + c_, mean_scale=3.0)[0] for c_ in range(nm)])
    sig = np.array([1.0, 1.2])
    cs = rng.standard_normal((nm, d, k))
    ms = rng.standard_normal((nm, d))
    lw = np.log(np.array([0.4, 0.6]))
    ds = P.Dataset(x)
    mix = P.PPCAMix([P.PPCAModel(sig[c_], cs[c_], ms[c_]) for c_ in range(nm)], lw)
    for _ in range(2):
        sig, cs, ms, lw = oracle.mix_iterate(x, sig, cs, ms, lw)
        mix = mix.iterate(ds)
        for c_, mdl in enumerate(mix.models):
            assert abs(mdl.isotropic_noise - sig[c_]) < RTOL * sig[c_]
            assert _rel(mdl.transform, cs[c_]) < RTOL and _rel(mdl.mean, ms[c_]) < RTOL
        assert _rel(mix.log_weights, lw) < RTOL
