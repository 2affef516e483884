"""The fused EM pass at the shapes where the hand-offs between its front waves can go wrong (ppca_em9.hip: the one-way signal
`solved` and the per-wave adds to `wready` in place of the front role's barrier behind phase beta; the protocol itself is walked
on the CPU in test_em_role_sync_host.py).  Who waits for whom changes nothing that is computed, so every case is the pass against the CPU
oracle: the raw statistics block by block at 1e-9, then two EM steps at RTOL.

Shapes: workgroups that walk 0, 1, 2, 3, 5, 6, 8, 10, 19 and 38 tiles (grid limits 1, 2 and 4 at n = 32 * 37 + 5 and at
n = 5 * 32 + 7, one workgroup at n = 5 * 32, the full grid at n = 1 000) -- with 38 tiles in one workgroup every wave is the solver
nine times and a wave that runs ahead meets every counter's wrap of buffer parity and mask slot; k = 1 (no column pairs, idle
half-waves), 2 and 4 (row-major factor), 6, 7 and 10 (entry-major factor; 10: the squeezed row); d = 256, 200 and 5; weights; the
mixture's gathered weighted pass; an all-masked row in every data set; the back role's cold paths (a row that goes round the
fixed-point form, then a rise of the exponents and a second cut) while the front runs ahead; and the 38-tile pass ten times, bit
for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # north_star tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@pytest.fixture()
def ctx(P):
    from ppca_rs_amd import _lib

    c = _lib.default_context()
    c.set_grid_limit(0)
    c.set_heavy_rows(8)
    c.debug_counters(reset=True)
    yield c
    c.set_grid_limit(0)
    c.set_heavy_rows(8)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _blocks(d, k, n):
    kp = k * (k + 1) // 2
    bounds = [0, d * k, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d, 2 * d * k + d * kp + 2 * d, n]
    return list(zip(["cross", "S", "U", "sumx", "totals", "scalars"], bounds[:-1], bounds[1:]))


def _stats_raw(ds, m, d, k):
    from ppca_rs_amd import _lib

    got = np.empty(_lib.lib().ppca_stats_len(d, k))
    _lib.check(_lib.lib().ppca_stats_raw(ds._ctx.handle, ds._h, m._device(ds._ctx).h, _lib.ptr(got)))
    return got


def _check_pass(P, oracle, ds, x, w, d, k, seed, tag):
    """ds holds the rows x (weights w or None): raw statistics and two EM steps against the oracle."""
    x = np.ascontiguousarray(x)
    rng = np.random.default_rng(seed)
    c, mu, s = rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d), 0.7
    m = P.PPCAModel(s, c, mu)
    got = _stats_raw(ds, m, d, k)
    want = oracle.stats(x, s, c, mu, w)
    for name, a, b in _blocks(d, k, got.size):
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
    x[10] = np.nan  # an all-masked row
    return x


N38 = 32 * 37 + 5  # 38 tiles, the last of 5 rows
N6 = 5 * 32 + 7    # 6 tiles, the last of 7 rows

# (n, d, k, grid limit, weighted)
CASES = [
    (61, 256, 10, 1, False),    # one workgroup, two tiles: the smallest case (first in the file)
    (N6, 256, 10, 4, False),    # 2, 2, 2 and 0 tiles
    (N6, 256, 10, 2, False),    # 3 and 3
    (N6, 256, 10, 1, False),    # 6
    (160, 256, 10, 1, False),   # 5, all full
    (1000, 256, 10, 0, False),  # the full grid: one tile or none per workgroup
    (N38, 256, 10, 1, False),   # 38: every wave the solver nine times
    (N38, 256, 10, 2, False),   # 19 and 19
    (N38, 256, 10, 4, False),   # 10, 10, 10 and 8
    (N38, 200, 1, 1, False),
    (N38, 5, 2, 1, False),
    (N38, 200, 6, 1, False),
    (N38, 256, 7, 2, False),
    (N6, 5, 1, 4, False),
    (N6, 200, 2, 2, False),
    (N6, 256, 4, 1, False),
    (N6, 5, 6, 2, False),
    (N6, 200, 7, 4, False),
    (1000, 200, 7, 0, False),
    (1000, 5, 1, 0, False),
    (N38, 256, 10, 1, True),    # weighted
    (N6, 200, 6, 4, True),
]


@pytest.mark.parametrize("n,d,k,limit,weighted", CASES, ids=["n%d-d%d-k%d-g%d%s" % (c[0], c[1], c[2], c[3], "-w" if c[4] else "") for c in CASES])
def test_pass_against_oracle(P, oracle, ctx, n, d, k, limit, weighted):
    x = _data(oracle, n, d, k, 9000 + n + d + k)
    w = np.random.default_rng(n + d).uniform(0.5, 1.5, n) if weighted else None
    ctx.set_grid_limit(limit)
    _check_pass(P, oracle, P.Dataset(x, w), x, w, d, k, 29 * d + k, (n, d, k, limit, weighted))


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


@pytest.mark.parametrize("heavy_max", [8, 0])
def test_cold_paths_of_the_back_role(P, oracle, ctx, heavy_max):
    """Row 70 of n = 200 (third of seven tiles of ONE workgroup) at 1e6 x its neighbours.  heavy_max = 8: the row goes round the
    fixed-point form (heavy bits, a second cut of the tile, heavy_add: three more barriers of the back role) and no exponent rises;
    heavy_max = 0: the exponents rise and the tile is cut again.  Either way the back role holds the tile's W rows far longer than
    usual while the front role runs ahead, and must find them, and the sample masks, untouched: every block within 1e-9 of the
    oracle and, where the large row is masked, the diagonal of S dimension by dimension (the tolerances of
    test_outlier_rows_go_round_the_fixed_point_form)."""
    n, d, k = 200, 256, 10
    rng = np.random.default_rng(31 + k)
    x, _, _ = oracle.synth(n, d, k, 0.3, 19)
    x[70] *= 1e6
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.05 * rng.standard_normal(d), 0.7
    m = P.PPCAModel(s, c, mu)
    kp = k * (k + 1) // 2
    diag = [a * (a + 1) // 2 + a for a in range(k)]
    want = oracle.stats(x, s, c, mu, None)
    ctx.set_grid_limit(1)
    ctx.set_heavy_rows(heavy_max)
    ctx.debug_counters(reset=True)
    got = _stats_raw(P.Dataset(x), m, d, k)
    cnt = ctx.debug_counters()
    if heavy_max:
        assert ctx.last_guard() == (0, 0) and ctx.last_fallback()[:3] == (0, 0, 0), ctx.last_guard()
        assert cnt[0] == 0, cnt
    else:
        assert cnt[0] >= 1, cnt  # the exponents rose and the tile was cut a second time
    for name, a, b in _blocks(d, k, got.size):
        assert _rel(got[a:b], want[a:b]) < 1e-9, (heavy_max, name)
    Sg, Sw = got[d * k:d * k + d * kp].reshape(d, kp), want[d * k:d * k + d * kp].reshape(d, kp)
    masked = ~np.isfinite(x[70])
    assert masked.any()
    assert (np.abs(Sg[masked][:, diag] - Sw[masked][:, diag]) / np.abs(Sw[masked][:, diag])).max() < 1e-9, heavy_max


def test_the_38_tile_pass_repeats_bit_for_bit(P, oracle, ctx):
    """One workgroup, 38 tiles, k = 10, d = 256, ten times: ppca_stats_raw identical to the last bit (a race shows here first)."""
    d, k = 256, 10
    x = _data(oracle, N38, d, k, 4242)
    rng = np.random.default_rng(5)
    m = P.PPCAModel(0.7, rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d))
    ds = P.Dataset(x)
    ctx.set_grid_limit(1)
    first = _stats_raw(ds, m, d, k)
    assert np.isfinite(first).all()
    for rep in range(9):
        assert np.array_equal(_stats_raw(ds, m, d, k), first), rep
