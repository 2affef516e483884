"""The pairwise second moments of a masked dataset on the GPU (ppca_dataset_pairwise_moments, one dense fp64 MFMA pass) against the
row-by-row numpy restatement (tests/moments_restatement.py), and the spectral starts built on them (method="pca", init="pca").

Tolerance of the pass: the error of each matrix relative to the largest magnitude in the reference matrix is below 1e-11 -- the
worst-case rounding of a sum of n fp64 products is about n 2^-53 of the largest diagonal entry whatever the order (6e-13 at
n = 5000); the margin covers the rounding of x - b.  Each check prints its worst error before asserting."""
import functools

import numpy as np
import pytest

import fa_restatement as FR
import moments_restatement as R

pytestmark = pytest.mark.gpu

TOL = 1e-11
SHAPES = [(1, 1), (3, 5), (65, 17), (1000, 64), (1000, 65), (257, 130), (600, 256), (300, 300)]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@functools.lru_cache(maxsize=None)
def _case(n, d, weights):
    """(x, w or None, centre, reference (sums, counts, cross)): 30 % masked, one fully masked column and one fully masked row, two
    columns never observed together, a few +-inf entries (ingest masks them) -- each where the shape has room for it.  Computed once
    per (shape, weights) and shared; nobody writes to it."""
    rng = np.random.default_rng(1000 * n + d)
    x = rng.standard_normal((n, d)) * rng.uniform(0.1, 10.0, d) + 3.0 * rng.standard_normal(d)
    if n > 1:
        x[rng.random((n, d)) < 0.3] = np.nan
    if d >= 2 and n >= 2:  # columns 0 and 1 are never observed together
        half = np.arange(n) % 2 == 0
        x[half, 0] = np.nan
        x[~half, 1] = np.nan
    if d >= 4:
        x[:, d - 2] = np.nan  # a fully masked column
    if n >= 3:
        x[n // 2] = np.nan  # a fully masked row
        x[0, d - 1], x[n - 1, d // 2] = np.inf, -np.inf
    w = {"none": None, "int": rng.integers(0, 4, n).astype(np.float64), "real": rng.uniform(0.25, 2.0, n)}[weights]
    center = 3.0 * rng.standard_normal(d)
    ref = R.moments(x, w, center)
    for a in (x, center) + ref + (() if w is None else (w,)):
        a.setflags(write=False)
    return x, w, center, ref


def _rel(got, want):
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0))


@pytest.mark.parametrize("cross", [False, True], ids=["sym", "cross"])
@pytest.mark.parametrize("weights", ["none", "int", "real"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pass_against_restatement(P, shape, weights, cross):
    n, d = shape
    x, w, center, (sums, counts, crs) = _case(n, d, weights)
    ds = P.Dataset(np.array(x), None if w is None else np.array(w))
    got = ds.pairwise_moments(center, cross=cross)
    assert np.array_equal(got.center, center)
    errs = {"sums": _rel(got.sums, sums), "counts": _rel(got.counts, counts)}
    if cross:
        errs["cross"] = _rel(got.cross, crs)
    else:
        assert got.cross is None
    print(f"{n} x {d}, weights {weights}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e})")
    assert max(errs.values()) < TOL
    if weights != "real":
        assert np.array_equal(got.counts, counts)  # an exact integer contraction
    assert np.array_equal(got.sums, got.sums.T) and np.array_equal(got.counts, got.counts.T)  # bit for bit
    if d >= 2 and n >= 2:  # never observed together: exactly nothing
        for m in (got.sums, got.counts) + ((got.cross,) if cross else ()):
            assert m[0, 1] == 0.0 and m[1, 0] == 0.0
    if d >= 4:  # the fully masked column
        for m in (got.sums, got.counts) + ((got.cross,) if cross else ()):
            assert np.all(m[d - 2] == 0.0) and np.all(m[:, d - 2] == 0.0)
    # the diagonals are the column sums of the streaming pass
    tot, sm, sq = ds._scale_columns(np.ones(d), center, out=False, col_sums=True)[1]
    assert np.abs(np.diag(got.counts) - tot).max() <= 1e-12 * max(np.abs(tot).max(), 1.0)
    assert np.abs(np.diag(got.sums) - sq).max() <= 1e-12 * max(np.abs(sq).max(), 1.0)
    if cross:
        scale = np.abs(np.where(np.isfinite(x), x - center, 0.0)).sum(0).max()
        assert np.abs(np.diag(got.cross) - sm).max() <= 1e-12 * max(scale, 1.0)


def test_centred_on_the_means(P):
    """Columns with mean 1e6 and unit spread: the centring happens before the product, so nothing cancels."""
    rng = np.random.default_rng(77)
    n, d = 1000, 65
    x = 1e6 + rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    w = rng.uniform(0.25, 2.0, n)
    ds = P.Dataset(x, w)
    got = ds.pairwise_moments(cross=True)  # center="mean"
    mean = R.column_means(x, w)
    assert np.abs(got.center - mean).max() <= 1e-12 * 1e6
    sums, counts, crs = R.moments(x, w, got.center)
    errs = (_rel(got.sums, sums), _rel(got.counts, counts), _rel(got.cross, crs))
    print("mean 1e6, unit spread: sums %.2e counts %.2e cross %.2e (bound %.0e)" % (errs + (TOL,)))
    assert max(errs) < TOL
    assert np.abs(sums).max() < 2.0 * w.sum()  # (unit spread: the reference itself is of order n, not n 1e12)
    # the shortcuts
    assert np.array_equal(ds.covariance(), got.covariance(), equal_nan=True)
    assert np.array_equal(ds.covariance("pairwise", ddof=1.0), got.covariance("pairwise", 1.0), equal_nan=True)
    assert np.array_equal(ds.correlation(), got.correlation(), equal_nan=True)
    zero = ds.pairwise_moments(center=None)
    assert np.array_equal(zero.center, np.zeros(d)) and _rel(zero.counts, counts) < TOL
    with pytest.raises(ValueError):
        ds.pairwise_moments(center=np.full(d, np.nan))
    with pytest.raises(ValueError):
        ds.pairwise_moments(center=np.zeros(d + 1))


def test_row_splits_and_reproducibility(P):
    """n = 5000, d = 64 (one tile pair; six jobs per workgroup of the grid).  Grid limit 1: 6 jobs of 53 row steps; limit 3: 18 jobs
    of 18 steps; the default grid: 313 jobs of one step each, 313 partials per element."""
    rng = np.random.default_rng(5)
    n, d = 5000, 64
    x = rng.standard_normal((n, d)) * rng.uniform(0.1, 10.0, d)
    x[rng.random((n, d)) < 0.3] = np.nan
    w = rng.uniform(0.25, 2.0, n)
    ds = P.Dataset(x, w)
    center = R.column_means(x, w)
    ref = R.moments(x, w, center)
    ctx = ds._ctx
    res = {}
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            a, b = ds.pairwise_moments(center, cross=True), ds.pairwise_moments(center, cross=True)
            for name, want in zip(("sums", "counts", "cross"), ref):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (limit, name)  # two calls on one grid: bit-identical
                err = _rel(getattr(a, name), want)
                print(f"grid limit {limit}: {name} {err:.2e}")
                assert err < TOL
            res[limit] = a
    finally:
        ctx.set_grid_limit(0)
    for limit in (1, 3):
        for name in ("sums", "counts", "cross"):
            assert _rel(getattr(res[limit], name), getattr(res[0], name)) <= 1e-12, (limit, name)


def test_additive_over_chunks_and_empty(P):
    rng = np.random.default_rng(9)
    n, d = 1001, 70
    x = rng.standard_normal((n, d)) + rng.standard_normal(d)
    x[rng.random((n, d)) < 0.3] = np.nan
    ds = P.Dataset(x, rng.uniform(0.25, 2.0, n))
    whole = ds.pairwise_moments(cross=True)
    halves = [c.pairwise_moments(whole.center, cross=True) for c in ds.chunks(2)]
    assert len(halves) == 2
    both = halves[0] + halves[1]
    for name in ("sums", "counts", "cross"):
        assert _rel(getattr(both, name), getattr(whole, name)) <= 1e-12, name
    empty = ds._slice(0, 0).pairwise_moments(whole.center, cross=True)
    for name in ("sums", "counts", "cross"):
        assert np.array_equal(getattr(empty, name), np.zeros((d, d))), name
    assert np.array_equal(ds._slice(5, 0).pairwise_moments().center, np.zeros(d))


# --------------------------------------------------------------------------- the starts
def _host_moments(P, x):
    c = R.column_means(x)
    return P.PairwiseMoments(c, *R.moments(x, None, c))


def test_pca_start_is_from_moments(P, oracle):
    x, _, _ = oracle.synth(500, 9, 3, 0.3, 11)
    x[:, 5] = np.nan
    ds = P.Dataset(x)
    want = P.PPCAModel.from_moments(3, _host_moments(P, x))
    got = P.PPCAModel.init(3, ds, method="pca")
    errs = (np.abs(got.transform - want.transform).max() / np.abs(want.transform).max(),
            abs(got.isotropic_noise / want.isotropic_noise - 1.0), np.abs(got.mean - want.mean).max() / np.abs(want.mean).max())
    print("method='pca' against from_moments of the restatement: C %.2e sigma %.2e mean %.2e" % errs)
    assert max(errs) < 1e-9
    assert np.all(got.transform[5] == 0.0) and got.mean[5] == 0.0
    fw, fg = P.FAModel.from_moments(3, _host_moments(P, x)), P.FAModel.init(3, ds, method="pca")
    assert np.abs(fg.transform - fw.transform).max() < 1e-9 * np.abs(fw.transform).max()
    assert np.abs(fg.noise / fw.noise - 1.0).max() < 1e-9 and np.abs(fg.mean - fw.mean).max() < 1e-9 * np.abs(fw.mean).max()


def test_pca_start_is_stationary_on_complete_data(P, oracle):
    """|llk(m.iterate(ds)) - llk(m)| <= 1e-7 |llk|: the device EM step is held to the oracle at 1e-5 relative by the parity tests, and
    at a stationary point the llk is second order in a parameter error; 1e-7 leaves three orders of margin over (1e-5)^2."""
    x, _, _ = oracle.synth(2000, 12, 3, 0.0, 7)
    ds = P.Dataset(x)
    m = P.PPCAModel.init(3, ds, method="pca")
    l0, l1 = m.llk(ds), m.iterate(ds).llk(ds)
    print("complete data: llk", l0, "after one device EM step", l1, "relative", abs(l1 - l0) / abs(l0))
    assert abs(l1 - l0) <= 1e-7 * abs(l0)


@pytest.mark.parametrize("case", [(4000, 24, 4, 0.3, 21), (3000, 40, 6, 0.5, 22), (5000, 16, 2, 0.3, 23)], ids=lambda c: "%dx%d-k%d" % c[:3])
def test_pca_start_saves_ppca_iterations(P, oracle, case):
    """llk(pca start + 3 EM iterations) >= llk(PPCAModel.init(k, ds, seed) + 20 EM iterations), all on the device.

    Data: oracle.synth(n, d, k, p, seed, sigma_true=0.5); the random start is PPCAModel.init(k, ds, seed=seed), the same seed.  On
    the CPU oracle with that exact draw, llk per row:

        (n, d, k, p, seed)        pca start   pca + 3    random + 20   margin
        (4000, 24, 4, 0.3, 21)    -19.8886    -19.8186   -19.8498      0.0311
        (3000, 40, 6, 0.5, 22)    -27.4033    -27.0245   -27.0976      0.0731
        (5000, 16, 2, 0.3, 23)    -11.7608    -11.7539   -11.7673      0.0134

    every margin above the 0.01 per row that keeps the comparison clear of the device's 1e-5 parity tolerance."""
    n, d, k, p, seed = case
    x, _, _ = oracle.synth(n, d, k, p, seed, sigma_true=0.5)
    ds = P.Dataset(x)
    a = P.PPCAModel.init(k, ds, method="pca")
    for _ in range(3):
        a = a.iterate(ds)
    b = P.PPCAModel.init(k, ds, seed=seed)
    for _ in range(20):
        b = b.iterate(ds)
    la, lb = a.llk(ds) / n, b.llk(ds) / n
    print(f"{case}: pca + 3 {la:.4f}, random + 20 {lb:.4f} per row")
    assert la >= lb


@pytest.mark.parametrize("case", [(1200, 12, 3, 0.3, 31), (1000, 10, 2, 0.4, 32)], ids=lambda c: "%dx%d-k%d" % c[:3])
def test_pca_start_saves_fa_iterations(P, case):
    """llk(FAModel.init(method="pca") + 3 ECM iterations) >= llk(FAModel.init(seed=seed) + 10), all on the device.

    Data: psi = exp(default_rng(seed).uniform(ln 1e-2, ln 1e2, d)), fa_restatement.synth(n, d, k, psi, p, seed).  On the CPU
    restatement (fa_restatement.iterate) with the exact draw of FAModel.init(seed=seed), llk per row:

        (n, d, k, p, seed)        pca + 3     random + 10   margin
        (1200, 12, 3, 0.3, 31)    -14.7036    -14.7434      0.0398
        (1000, 10, 2, 0.4, 32)    -16.5268    -16.5505      0.0238"""
    n, d, k, p, seed = case
    psi = np.exp(np.random.default_rng(seed).uniform(np.log(1e-2), np.log(1e2), d))
    x, _, _ = FR.synth(n, d, k, psi, p, seed)
    ds = P.Dataset(x)
    a = P.FAModel.init(k, ds, method="pca")
    for _ in range(3):
        a = a.iterate(ds)
    b = P.FAModel.init(k, ds, seed=seed)
    for _ in range(10):
        b = b.iterate(ds)
    la, lb = a.llk(ds) / n, b.llk(ds) / n
    print(f"{case}: pca + 3 {la:.4f}, random + 10 {lb:.4f} per row")
    assert la >= lb


def test_trainers_take_the_start(P, oracle):
    x, _, _ = oracle.synth(800, 11, 3, 0.3, 41)
    ds = P.Dataset(x)
    got = P.PPCATrainer(ds).train(state_size=3, n_iters=3, init="pca", quiet=True)
    m = P.PPCAModel.init(3, ds, method="pca")
    for _ in range(3):
        m = m.iterate(ds)
    want = m.to_canonical()
    assert np.abs(got.transform - want.transform).max() <= 1e-12 * np.abs(want.transform).max()
    assert abs(got.isotropic_noise - want.isotropic_noise) <= 1e-12 * want.isotropic_noise
    assert np.abs(got.mean - want.mean).max() <= 1e-12 * np.abs(want.mean).max()
    # `start` wins over `init`; the FA trainer takes the same keyword
    start = P.PPCAModel.init(3, ds, seed=4)
    kept = P.PPCATrainer(ds).train(start=start, state_size=3, n_iters=0, init="pca", quiet=True)
    assert np.array_equal(kept.transform, start.to_canonical().transform)
    fa = P.FATrainer(ds).train(state_size=3, n_iters=0, init="pca", quiet=True)
    fw = P.FAModel.init(3, ds, method="pca").to_canonical()
    assert np.array_equal(fa.transform, fw.transform) and np.array_equal(fa.noise, fw.noise)
