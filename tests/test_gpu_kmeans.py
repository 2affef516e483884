"""Masked k-means on the GPU (ppca_dataset_kmeans_step: one Lloyd iteration in one read of the dataset; ppca_dataset_kmeans_seed:
k-means++ on the device) against the row-by-row numpy restatement (tests/kmeans_restatement.py), and the mixture starts built on it
(method="kmeans", init="kmeans").

Labels are compared on EVERY row: before a comparison the restatement's relative gap (second-smallest minus smallest distance over
the row's largest) is asserted to be at least 1e-9 on every row that observes anything -- seven orders above the rounding of a
distance -- so that no label can differ by rounding; a row with no observed entry is an exact tie (all distances 0) and must get label
0.  Tolerance of dist, sums and inertia: below 1e-11 of the largest magnitude in the reference array, the bound of
tests/test_gpu_pairwise_moments.py (a sum of n fp64 terms rounds at about n 2^-53 of the largest term whatever the order, 1e-13 at
n = 1000; the margin covers the rounding of x - mu).  Each check prints its worst error before asserting."""
import functools

import numpy as np
import pytest

import famix_restatement as FM
import kmeans_restatement as KR
import mask_patterns as MP

pytestmark = pytest.mark.gpu

TABLE, FA_CASE, fa_case_psi = KR.TABLE, KR.FA_CASE, KR.fa_case_psi
TOL = 1e-11
GAP = 1e-9
SHAPES = [(1, 1), (3, 5), (65, 17), (257, 64), (1000, 130), (600, 256), (300, 512), (300, 514), (200, 1030)]
KS = [1, 2, 3, 8, 9, 16]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(got, want):
    scale = np.abs(want).max()
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0))


@functools.lru_cache(maxsize=None)
def _data(n, d, weights):
    """(x, w or None, column offsets, column spreads): 30 % masked, a fully masked row and column, one column with mean 1e6 and unit
    spread, +-inf entries (ingest masks them) -- each where the shape has room for it.  Shared, read-only."""
    rng = np.random.default_rng(1000 * n + d)
    spread, offset = rng.uniform(0.1, 10.0, d), 3.0 * rng.standard_normal(d)
    if d >= 3:
        spread[1], offset[1] = 1.0, 1e6
    x = rng.standard_normal((n, d)) * spread + offset
    if n > 1:
        x[rng.random((n, d)) < 0.3] = np.nan
    if d >= 4:
        x[:, d - 2] = np.nan
    if n >= 3:
        x[n // 2] = np.nan
        x[0, d - 1], x[n - 1, d // 2] = np.inf, -np.inf
    w = {"none": None, "int": rng.integers(0, 4, n).astype(np.float64), "real": rng.uniform(0.25, 2.0, n)}[weights]
    for a in (x, spread, offset) + (() if w is None else (w,)):
        a.setflags(write=False)
    return x, w, offset, spread


@functools.lru_cache(maxsize=None)
def _case(n, d, nc, weights, scaled):
    """The data, nc continuous random centres, the scale and the restatement's step: once per case, shared, read-only."""
    x, w, offset, spread = _data(n, d, weights)
    rng = np.random.default_rng(7 * n + 13 * d + nc)
    centers = offset + spread * rng.standard_normal((nc, d))
    scale = np.exp(rng.uniform(-2.0, 2.0, d)) if scaled else None
    ref = KR.step(x, w, centers, scale)
    for a in (centers,) + ref[:4] + (ref[5],) + (() if scale is None else (scale,)):
        a.setflags(write=False)
    return x, w, centers, scale, ref


def _check_step(P, x, w, centers, scale, ref, tag, int_weights=False):
    """One device step against the restatement's: labels on all rows (after the gap condition), dist / sums / inertia at TOL."""
    labels, dist, tot, sums, inertia, dm = ref
    some = np.isfinite(x).any(axis=1)
    gaps = KR.relative_gaps(dm)
    assert gaps[some].min(initial=np.inf) >= GAP, (tag, "the case has a near tie: change its seed")
    assert np.all(labels[~some] == 0) and np.all(dist[~some] == 0.0)
    ds = P.Dataset(np.array(x), None if w is None else np.array(w))
    got = ds.kmeans_step(centers, scale, labels=True, distances=True)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels), tag
    errs = dict(dist=_rel(got.distances, dist), tot=_rel(got.totals, tot), sums=_rel(got.sums, sums),
                inertia=abs(got.inertia - inertia) / max(abs(inertia), 1e-300) if inertia > 0 else abs(got.inertia))
    print(tag, " ".join("%s %.1e" % kv for kv in errs.items()), "reads", got.reads, "smallest gap %.1e" % gaps[some].min(initial=np.inf))
    assert max(errs.values()) < TOL, (tag, errs)
    if int_weights:
        assert np.array_equal(got.totals, tot)
    assert np.abs(got.centers() - KR.new_centers(centers, tot, sums)).max() <= TOL * np.abs(centers).max()
    return ds, got


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("weights", ["none", "int", "real"])
@pytest.mark.parametrize("nc", KS, ids=lambda k: "K%d" % k)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_step_against_restatement(P, shape, nc, weights, scaled):
    n, d = shape
    x, w, centers, scale, ref = _case(n, d, nc, weights, scaled)
    ds, got = _check_step(P, x, w, centers, scale, ref, (n, d, nc, weights, scaled), int_weights=weights != "real")
    if d <= 512 and nc <= 8:
        assert got.reads == 1
    else:
        assert got.reads >= 2
    # the labelling alone (no sums): the same labels and distances, one read whenever K <= 8
    lab = ds._kmeans_call(np.array(centers), None if scale is None else np.array(scale), True, True, False)
    assert lab.totals is None and np.array_equal(lab.labels, ref[0]) and _rel(lab.distances, ref[1]) < TOL
    assert abs(lab.inertia - got.inertia) <= 1e-12 * max(abs(got.inertia), 1e-300)
    assert lab.reads == (1 if nc <= 8 else 2)


def test_exact_ties_and_degenerate_inputs(P):
    x, w, offset, spread = _data(1000, 130, "real")
    rng = np.random.default_rng(3)
    base = offset + spread * rng.standard_normal((3, 130))
    ds = P.Dataset(np.array(x), np.array(w))
    # two identical centres: the higher index gets no row
    twice = np.vstack([base[:1], base[:1], base[1:]])
    got = ds.kmeans_step(twice)
    assert not np.any(got.labels == 1) and np.all(got.totals[1] == 0.0) and np.all(got.sums[1] == 0.0) and np.any(got.labels == 0)
    assert np.array_equal(got.labels, KR.step(x, w, twice)[0])
    assert np.array_equal(got.centers()[1], twice[1])
    # a centre that no row is nearest to keeps its value
    far = np.vstack([base, offset + 1e4 * spread])
    got = ds.kmeans_step(far)
    assert not np.any(got.labels == 3) and np.array_equal(got.centers()[3], far[3])
    # a cluster that never observes a column keeps that column of its centre (column d - 2 is masked in every row)
    assert np.all(got.totals[:, 128] == 0.0) and np.array_equal(got.centers()[:, 128], far[:, 128])
    xc = np.array(x)
    for _ in range(20):  # (masking an entry can move its row to another cluster: until the rows of cluster 1 are settled)
        lab = KR.step(xc, w, base)[0]
        if not np.isfinite(xc[lab == 1, 5]).any():
            break
        xc[lab == 1, 5] = np.nan
    else:
        raise AssertionError("the rows of cluster 1 did not settle")
    got = P.Dataset(xc, np.array(w)).kmeans_step(base)
    assert np.array_equal(got.labels, lab)
    assert np.any(got.labels == 1) and got.totals[1, 5] == 0.0 and got.centers()[1, 5] == base[1, 5] and got.totals[0, 5] > 0.0
    # a zero-row slice gives zeros
    for empty in (ds._slice(0, 0), ds._slice(7, 0)):
        z = empty.kmeans_step(base, distances=True)
        assert z.labels.shape == (0,) and z.distances.shape == (0,) and z.inertia == 0.0 and z.reads == 0
        assert np.all(z.totals == 0.0) and np.all(z.sums == 0.0) and np.array_equal(z.centers(), base)
    # K = 1 reproduces the column means after one step from any start
    _, mean, _ = ds.column_stats()
    live = np.arange(130) != 128
    for start in (np.zeros((1, 130)), base[:1], offset[None, :] + 100.0 * spread):
        c1 = ds.kmeans_step(start).centers()[0]
        err = (np.abs(c1 - mean) / np.maximum(np.abs(mean), spread))[live].max()  # per column, in the column's own size
        print("K = 1 against column_stats, worst column: %.1e" % err)
        assert err <= 1e-12 and c1[128] == start[0, 128]
    with pytest.raises(P.PPCAError):
        ds._kmeans_call(np.zeros((17, 130)), None, True, False, True)  # the library's own range check: unsupported


def test_grid_and_reproducibility(P):
    """n = 5000, d = 64, K = 8 (32 threads per row, 8 row groups of 4 rows in flight: 32 rows per step).  The grid limit caps the
    launch itself: limit 1 is ONE workgroup walking all 157 row steps, limit 3 three of 53; the default grid (two workgroups per CU,
    512 on 256 CUs) has 10 rows each.  labels and dist depend on their row alone."""
    rng = np.random.default_rng(5)
    n, d, nc = 5000, 64, 8
    spread = rng.uniform(0.1, 10.0, d)
    x = rng.standard_normal((n, d)) * spread
    x[rng.random((n, d)) < 0.3] = np.nan
    w = rng.uniform(0.25, 2.0, n)
    centers = spread * rng.standard_normal((nc, d))
    ref = KR.step(x, w, centers)
    ds = P.Dataset(x, w)
    ctx = ds._ctx
    res = {}
    try:
        for limit in (1, 3, 0):
            ctx.set_grid_limit(limit)
            a, b = [ds.kmeans_step(centers, distances=True) for _ in range(2)]
            for name in ("labels", "distances", "totals", "sums"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (limit, name)  # two calls on one grid: bit-identical
            assert a.inertia == b.inertia and a.reads == 1
            assert np.array_equal(a.labels, ref[0])
            errs = (_rel(a.distances, ref[1]), _rel(a.totals, ref[2]), _rel(a.sums, ref[3]), abs(a.inertia / ref[4] - 1.0))
            print("grid limit %d: dist %.1e tot %.1e sums %.1e inertia %.1e" % ((limit,) + errs))
            assert max(errs) < TOL
            res[limit] = a
    finally:
        ctx.set_grid_limit(0)
    for limit in (1, 3):
        assert np.array_equal(res[limit].labels, res[0].labels) and np.array_equal(res[limit].distances, res[0].distances)  # bit for bit
        for name in ("totals", "sums"):
            assert _rel(getattr(res[limit], name), getattr(res[0], name)) <= 1e-12, (limit, name)
        assert abs(res[limit].inertia / res[0].inertia - 1.0) <= 1e-12
    halves = [c.kmeans_step(centers) for c in ds.chunks(2)]
    assert len(halves) == 2
    both = halves[0] + halves[1]
    assert both.labels is None
    for name in ("totals", "sums"):
        assert _rel(getattr(both, name), getattr(res[0], name)) <= 1e-12, name
    assert abs(both.inertia / res[0].inertia - 1.0) <= 1e-12
    assert np.array_equal(np.concatenate([h.labels for h in halves]), res[0].labels)


@pytest.mark.parametrize("name", MP.NAMES)
def test_mask_patterns(P, oracle, name):
    """Every structured pattern of tests/mask_patterns.py at n = 293, d = 130 with K = 3, weighted."""
    n, d, nc = 293, 130, 3
    x, w, _, _ = MP.case(oracle, n, d, 4, name, 3000 + d)
    centers = 0.7 * np.random.default_rng(d).standard_normal((nc, d))
    _check_step(P, x, w, centers, None, KR.step(x, w, centers), ("pattern", name))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("case", [(1000, 24, 5), (600, 130, 8)], ids=lambda c: "%dx%d-K%d" % c)
def test_seeding(P, case, weighted):
    """The chosen rows equal the restatement's (after asserting that every pick is at least 1e-9 of the total away from a boundary of
    the cumulative sum), and the centres are bit-equal to the restatement's run with the SAME column means.  A deviation from a plain
    bit-comparison of the two seedings, on purpose: a masked entry of a chosen row carries the weighted column mean, and the device's
    sums sweep and the row-by-row restatement add a column in different orders, so their means differ in the last bits.  The
    restatement is therefore run twice: with its own means (the rows must agree, the centres to 1e-12 of the largest entry, and the
    device's means to 1e-12 of the restatement's) and with the device's means handed in (the whole centre bit for bit)."""
    n, d, nc = case
    x, w, _, _ = _data(n, d, "real" if weighted else "none")
    u = np.random.default_rng(100 + n).random(nc)
    centers, rows, margins = KR.seed(x, w, u)
    print("seeding", case, "weighted" if weighted else "plain", "rows", rows.tolist(), "smallest pick margin %.1e" % margins.min())
    assert margins.min() >= GAP, "a pick sits on a boundary: change the seed of u"
    ds = P.Dataset(np.array(x), None if w is None else np.array(w))
    got, got_rows = ds._kmeans_seed(nc, u, None)
    assert np.array_equal(got_rows, rows)
    assert np.abs(got - centers).max() <= 1e-12 * np.abs(centers).max()
    _, mean, _ = ds.column_stats()
    ref_mean = KR.R.column_means(x, w)
    assert np.abs(mean - ref_mean).max() <= 1e-12 * np.abs(ref_mean).max()
    same, same_rows, same_margins = KR.seed(x, w, u, means=mean)
    assert same_margins.min() >= GAP and np.array_equal(same_rows, rows)
    assert np.array_equal(got, same)  # the whole centre, bit for bit
    for c in range(nc):  # masked entries of a chosen row carry the column mean
        o = np.isfinite(x[rows[c]])
        assert o.any() and (~o).any() and np.array_equal(got[c, ~o], mean[~o]) and np.array_equal(got[c, o], x[rows[c], o])
    # under a scale the picks follow the scaled distances
    scale = np.exp(np.random.default_rng(d).uniform(-2.0, 2.0, d))
    _, rows_s, margins_s = KR.seed(x, w, u, scale)
    assert margins_s.min() >= GAP
    assert np.array_equal(ds._kmeans_seed(nc, u, scale)[1], rows_s)


@functools.lru_cache(maxsize=None)
def _table_data(case):
    n, d, k, nm, masked, seed, sep = case
    x = FM.synth(n, d, k, nm, np.ones(d), masked, seed, separation=sep)[0]
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "%dx%d-k%d-m%d" % c[:4])
def test_lloyd_against_restatement(P, case):
    n, d, k, nm, masked, seed, sep = case
    x = _table_data(case)
    ref = KR.lloyd(x, None, nm, np.random.default_rng(seed).random(nm))
    assert ref["min_gap"] >= GAP  # on every iteration's assignment
    km = P.Dataset(np.array(x)).kmeans(nm, seed=seed)
    h = km.history
    assert km.n_iters_run == len(h) == ref["n_iters_run"] and km.converged == ref["converged"]
    assert np.all(h[1:] <= h[:-1] * (1.0 + 1e-12)) and km.inertia <= h[-1] * (1.0 + 1e-12)
    errs = (_rel(km.centers, ref["centers"]), abs(km.inertia / ref["inertia"] - 1.0), _rel(h, ref["history"]))
    print(case, "centres %.1e inertia %.1e history %.1e; iterations %d, smallest gap %.1e" % (errs + (km.n_iters_run, ref["min_gap"])))
    assert np.array_equal(km.labels, ref["labels"]) and max(errs) < 1e-10
    assert np.abs(km.cluster_weights - ref["cluster_weights"]).max() == 0.0


def test_lloyd_converges_on_separated_blobs(P):
    rng = np.random.default_rng(61)
    n, d = 600, 8
    mus = 40.0 + 15.0 * np.arange(3)[:, None] + rng.uniform(-2, 2, (3, d))
    which = rng.integers(0, 3, n)
    x = mus[which] + rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.2] = np.nan
    w = rng.uniform(0.25, 2.0, n)
    ds = P.Dataset(x, w)
    km = ds.kmeans(3, seed=61)
    print("blobs: iterations", km.n_iters_run, "converged", km.converged, "weights", km.cluster_weights)
    assert km.converged and km.n_iters_run < 20
    assert len(km.history) == km.n_iters_run and abs(km.history[-1] / km.inertia - 1.0) <= 1e-12  # the last step moved nothing
    # the clusters are the blobs, up to their order
    for c in range(3):
        assert len(set(which[km.labels == c].tolist())) == 1
    # `start` replaces the seeding; n_iters = 0 labels only
    again = ds.kmeans(3, start=km.centers, n_iters=0)
    assert np.array_equal(again.labels, km.labels) and again.n_iters_run == 0 and not again.converged and again.inertia == km.inertia
    std = ds.kmeans(3, seed=61, scale="std")
    assert std.converged and abs(std.cluster_weights.sum() - w.sum()) <= 1e-12 * w.sum()


# --------------------------------------------------------------------------- the starts
def _signed(got, want):
    """Largest deviation of the columns of got from those of want up to each column's sign, relative to the largest entry."""
    err = np.minimum(np.abs(got - want).max(axis=-2), np.abs(got + want).max(axis=-2))
    return float(err.max() / np.abs(want).max())


def test_starts_are_the_restated_starts(P):
    n, d, k, nm, masked, seed, sep = TABLE[0]
    x = _table_data(TABLE[0])
    ref = KR.lloyd(x, None, nm, np.random.default_rng(seed).random(nm))
    assert ref["min_gap"] >= GAP
    want = KR.ppca_mix_start(P, x, None, ref["labels"], nm, k)
    got = P.PPCAMix.init(nm, k, P.Dataset(np.array(x)), seed=seed, method="kmeans")
    errs = [_signed(g.transform, m.transform) for g, m in zip(got.models, want.models)]
    errs += [_rel(g.mean, m.mean) for g, m in zip(got.models, want.models)]
    errs += [abs(g.isotropic_noise / m.isotropic_noise - 1.0) for g, m in zip(got.models, want.models)]
    errs.append(float(np.abs(got.log_weights - want.log_weights).max()))
    print("PPCAMix.init(method='kmeans') against the restated start: worst %.1e" % max(errs))
    assert max(errs) < 1e-9
    # the FA mixture, clustered in units of the columns' standard deviations
    n, d, k, nm, masked, seed, sep = FA_CASE
    x = FM.synth(n, d, k, nm, fa_case_psi(), masked, seed, separation=sep)[0]
    ref = KR.lloyd(x, None, nm, np.random.default_rng(seed).random(nm), scale=KR.column_std_scale(x))
    assert ref["min_gap"] >= GAP
    noise, cs, mus, lw = KR.fa_mix_start(P, x, None, ref["labels"], nm, k)
    fa = P.FAMix.init(nm, k, P.Dataset(x), seed=seed, method="kmeans")
    errs = [_signed(fa.transforms[c], cs[c]) for c in range(nm)] + [_rel(fa.means[c], mus[c]) for c in range(nm)]
    errs += [float(np.abs(fa.noise / noise - 1.0).max()), float(np.abs(fa.log_weights - lw).max())]
    print("FAMix.init(method='kmeans') against the restated start: worst %.1e" % max(errs))
    assert max(errs) < 1e-9


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "%dx%d-k%d-m%d" % c[:4])
def test_kmeans_start_saves_mixture_iterations(P, case):
    """llk(k-means start + 3 EM iterations) > llk(random start, same seed, + 20), all on the device; the CPU oracle's figures for the
    same cases are in tests/test_kmeans_host.py (margins of 0.03, 3.6 and 2.2 per row against the device's 1e-5 parity)."""
    n, d, k, nm, masked, seed, sep = case
    ds = P.Dataset(np.array(_table_data(case)))
    a = P.PPCAMix.init(nm, k, ds, seed=seed, method="kmeans")
    l0 = a.llk(ds) / n
    for _ in range(3):
        a = a.iterate(ds)
    b = P.PPCAMix.init(nm, k, ds, seed=seed)
    for _ in range(20):
        b = b.iterate(ds)
    la, lb = a.llk(ds) / n, b.llk(ds) / n
    print(f"{case}: k-means + 0 {l0:.4f}, k-means + 3 {la:.4f}, random + 20 {lb:.4f} per row")
    assert la > lb


def test_fa_mixture_start_and_column_units(P):
    """Noise levels spread over 1e4: FAMix.init(method="kmeans") + 3 ECM iterations beat the random start + 10 (CPU restatement:
    -15.6611 against -18.0698 per row, tests/test_kmeans_host.py); a column in other units changes neither the labels nor, after the
    log-Jacobian, the log-likelihood."""
    n, d, k, nm, masked, seed, sep = FA_CASE
    x = FM.synth(n, d, k, nm, fa_case_psi(), masked, seed, separation=sep)[0]
    ds = P.Dataset(x)
    a = P.FAMix.init(nm, k, ds, seed=seed, method="kmeans")
    for _ in range(3):
        a = a.iterate(ds)
    b = P.FAMix.init(nm, k, ds, seed=seed)
    for _ in range(10):
        b = b.iterate(ds)
    la, lb = a.llk(ds) / n, b.llk(ds) / n
    print(f"FA {FA_CASE}: k-means + 3 {la:.4f}, random + 10 {lb:.4f} per row")
    assert la > lb
    fac = np.ones(d)
    fac[3] = 1e3
    ds2 = P.Dataset(x * fac)
    assert np.array_equal(ds2.kmeans(nm, seed=seed, scale="std").labels, ds.kmeans(nm, seed=seed, scale="std").labels)
    l1 = P.FAMix.init(nm, k, ds, seed=seed, method="kmeans").iterate(ds).llk(ds)
    l2 = P.FAMix.init(nm, k, ds2, seed=seed, method="kmeans").iterate(ds2).llk(ds2) + np.isfinite(x[:, 3]).sum() * np.log(1e3)
    print("column 3 x 1e3: llk after one iteration %.6f against %.6f, relative %.1e" % (l2, l1, abs(l2 / l1 - 1.0)))
    assert abs(l2 - l1) <= 1e-9 * abs(l1)


def test_random_method_is_unchanged_and_trainers_take_the_start(P):
    n, d, k, nm, masked, seed, sep = TABLE[0]
    ds = P.Dataset(np.array(_table_data(TABLE[0])))
    a, b = P.PPCAMix.init(nm, k, ds, seed=seed), P.PPCAMix.init(nm, k, ds, seed=seed, method="random")
    for ma, mb in zip(a.models, b.models):
        assert np.array_equal(ma.transform, mb.transform) and ma.isotropic_noise == mb.isotropic_noise and np.array_equal(ma.mean, mb.mean)
    assert np.array_equal(a.log_weights, b.log_weights)
    fa, fb = P.FAMix.init(nm, k, ds, seed=seed), P.FAMix.init(nm, k, ds, seed=seed, method="random")
    assert np.array_equal(fa.transforms, fb.transforms) and np.array_equal(fa.noise, fb.noise) and np.array_equal(fa.means, fb.means)
    # the trainers: what the explicit loop returns
    got = P.PPCAMixTrainer(ds).train(n_models=nm, state_size=k, n_iters=2, seed=seed, init="kmeans", quiet=True)
    m = P.PPCAMix.init(nm, k, ds, seed=seed, method="kmeans")
    for _ in range(2):
        m = m.iterate(ds)
    want = m.to_canonical()
    for g, w_ in zip(got.models, want.models):
        assert np.array_equal(g.transform, w_.transform) and g.isotropic_noise == w_.isotropic_noise and np.array_equal(g.mean, w_.mean)
    assert np.array_equal(got.log_weights, want.log_weights)
    fgot = P.FAMixTrainer(ds).train(n_models=nm, state_size=k, n_iters=0, seed=seed, init="kmeans", quiet=True)
    fwant = P.FAMix.init(nm, k, ds, seed=seed, method="kmeans").to_canonical()
    assert np.array_equal(fgot.transforms, fwant.transforms) and np.array_equal(fgot.noise, fwant.noise)
    kept = P.PPCAMixTrainer(ds).train(start=a, n_models=nm, state_size=k, n_iters=0, init="kmeans", quiet=True)  # `start` wins
    assert np.array_equal(kept.models[0].transform, a.to_canonical().models[0].transform)
