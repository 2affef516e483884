"""CPU-only: the masked k-means surface (ppca_dataset_kmeans_step / _seed, Dataset.kmeans / kmeans_step, KMeans, KMeansStep, the
from_kmeans starts, method= / init= "kmeans") is exported and declared; the numpy restatement (tests/kmeans_restatement.py) has the
properties the device pass is held to; the argument errors that are raised before any device call; and the k-means start through the
restatement and the CPU oracle: start + 3 EM iterations of the mixture beat the random start + 20."""
import inspect
import os
import re

import numpy as np
import pytest

import famix_restatement as FM
import kmeans_restatement as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE, FA_CASE, fa_case_psi = KR.TABLE, KR.FA_CASE, KR.fa_case_psi


class _FakeDataset:
    """What the checks of Dataset.kmeans / kmeans_step and the random mixture start ask of a dataset, without a device."""

    def __init__(self, n, d):
        self._n, self._d = n, d

    def __len__(self):
        return self._n

    def output_size(self):
        return self._d

    def empty_dimensions(self):
        return []


def _blobs(n, d, nc, seed, mask=0.3, spread=1.0, sep=8.0):
    rng = np.random.default_rng(seed)
    mus = sep * rng.standard_normal((nc, d))
    which = rng.integers(0, nc, n)
    x = mus[which] + spread * rng.standard_normal((n, d))
    x[rng.random((n, d)) < mask] = np.nan
    return x, mus, which


def test_kmeans_entry_points_exported(hiplib):
    from ppca_rs_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppca_hip.h")).read(), flags=re.S)
    for name in ("ppca_dataset_kmeans_step", "ppca_dataset_kmeans_seed"):
        assert hasattr(hiplib, name)
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, header)
    assert hiplib.ppca_abi_version() == 6


def test_kmeans_python_surface():
    import ppca_rs
    import ppca_rs_amd as p

    for name in ("KMeans", "KMeansStep"):
        assert name in p.__all__ and getattr(ppca_rs, name) is getattr(p, name)
    for meth in ("kmeans", "kmeans_step"):
        assert callable(getattr(p.Dataset, meth, None)), meth
    sig = inspect.signature(p.Dataset.kmeans)
    assert sig.parameters["n_iters"].default == 20 and sig.parameters["seed"].default is None
    assert sig.parameters["scale"].default is None and sig.parameters["start"].default is None
    sig = inspect.signature(p.Dataset.kmeans_step)
    assert sig.parameters["labels"].default is True and sig.parameters["distances"].default is False
    for cls in (p.PPCAMix, p.FAMix):
        assert callable(getattr(cls, "from_kmeans", None))
        assert inspect.signature(cls.init).parameters["method"].default == "random"
    for cls in (p.PPCAMixTrainer, p.FAMixTrainer):
        assert inspect.signature(cls.train).parameters["init"].default == "random"
    for field in ("centers", "labels", "inertia", "history", "cluster_weights", "n_iters_run", "converged"):
        assert field in p.KMeans.__dataclass_fields__, field


def test_step_sums_add_over_row_blocks():
    from ppca_rs_amd import KMeansStep

    x, mus, _ = _blobs(300, 7, 3, 2)
    w = np.random.default_rng(2).uniform(0.5, 2.0, 300)
    _, _, tot, sums, inertia, _ = KR.step(x, w, mus)
    halves = [KR.step(x[s], w[s], mus) for s in (slice(0, 140), slice(140, 300))]
    a, b = [KMeansStep(mus, h[2], h[3], h[4], labels=h[0]) for h in halves]
    both = a + b
    assert both.labels is None
    assert np.abs(both.totals - tot).max() <= 1e-12 * tot.max() and np.abs(both.sums - sums).max() <= 1e-12 * np.abs(sums).max()
    assert abs(both.inertia - inertia) <= 1e-12 * inertia
    assert np.abs(both.centers() - KR.new_centers(mus, tot, sums)).max() <= 1e-12 * np.abs(mus).max()
    with pytest.raises(ValueError):
        a + KMeansStep(mus + 1.0, halves[1][2], halves[1][3], halves[1][4])


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_restated_inertia_never_increases(scaled):
    """Both halves of an iteration decrease J = sum_i w_i sum_j m_ij a_j^2 (x_ij - mu_{label_i, j})^2: the assignment by construction,
    the update because the weighted mean over the observed entries minimises every (c, j) term."""
    x, _, _ = _blobs(500, 9, 4, 3, sep=2.0)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.25, 2.0, 500)
    scale = np.exp(rng.uniform(-2.0, 2.0, 9)) if scaled else None
    res = KR.lloyd(x, w, 4, rng.random(4), n_iters=15, scale=scale)
    h = res["history"]
    assert len(h) >= 3 and h[0] > h[-1]
    assert np.all(h[1:] <= h[:-1] * (1.0 + 1e-12))
    assert res["inertia"] <= h[-1] * (1.0 + 1e-12)
    assert abs(res["cluster_weights"].sum() - w.sum()) <= 1e-12 * w.sum()


def test_restated_degenerate_inputs():
    x, mus, _ = _blobs(200, 5, 2, 4)
    x[17] = np.nan
    far = np.vstack([mus, np.full((1, 5), 1e3)])  # a centre no row is nearest to: it keeps its value
    labels, dist, tot, sums, _, dm = KR.step(x, None, far)
    assert labels[17] == 0 and dist[17] == 0.0 and KR.relative_gaps(dm)[17] == 0.0  # a row with no entry: label 0
    assert not np.any(labels == 2) and np.all(tot[2] == 0.0)
    assert np.array_equal(KR.new_centers(far, tot, sums)[2], far[2])
    twice = np.vstack([mus[:1], mus[:1], mus[1:]])  # two identical centres: every tie goes to the lower index
    labels, _, tot, _, _, _ = KR.step(x, None, twice)
    assert not np.any(labels == 1) and np.all(tot[1] == 0.0) and np.any(labels == 0)
    xc = x.copy()
    lab0 = KR.step(xc, None, mus)[0]
    xc[lab0 == 1, 3] = np.nan  # a cluster that never observes a column keeps that column of its centre
    labels, _, tot, sums, _, _ = KR.step(xc, None, mus)
    rows = labels == 1
    assert rows.any() and not np.isfinite(xc[rows, 3]).any()
    assert KR.new_centers(mus, tot, sums)[1, 3] == mus[1, 3]


def test_restated_seeding():
    x, _, _ = _blobs(400, 6, 3, 5)
    w = np.random.default_rng(5).uniform(0.25, 2.0, 400)
    u = np.array([0.3, 0.9, 0.05, 0.5])
    centers, rows, margins = KR.seed(x, w, u)
    assert np.isfinite(centers).all() and len(set(rows.tolist())) == 4 and np.all(margins > 0.0)
    cum = np.cumsum(w)
    assert cum[rows[0]] > u[0] * cum[-1] and (rows[0] == 0 or cum[rows[0] - 1] <= u[0] * cum[-1])
    g = np.array([np.average(x[np.isfinite(x[:, j]), j], weights=w[np.isfinite(x[:, j])]) for j in range(6)])
    for c, r in zip(centers, rows):
        o = np.isfinite(x[r])
        assert np.array_equal(c[o], x[r, o]) and np.allclose(c[~o], g[~o], rtol=1e-13)
    # every row on a centre already: the rule of centre 0
    same = np.tile(np.arange(3.0), (10, 1))
    _, rows, _ = KR.seed(same, None, np.array([0.05, 0.55]))
    assert rows.tolist() == [0, 5]


def test_argument_errors_before_any_device_call():
    from ppca_rs_amd import Dataset

    class _NoDevice(Dataset):
        """A Dataset of a given shape that owns nothing on a device: any device call through it fails on its missing handle."""

        def __init__(self, n, d):
            self._n, self._dd = n, d

        def __len__(self):
            return self._n

        _d = property(lambda self: self._dd)

    ds = _NoDevice(50, 4)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            Dataset.kmeans(ds, bad)
    for bad in (2.5, "3", None, True):
        with pytest.raises(TypeError):
            Dataset.kmeans(ds, bad)
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 3, start=np.zeros((2, 4)))          # not (K, d)
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, start=np.zeros((2, 5)))
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, start=np.array([[0.0, 0.0, np.nan, 0.0], [1.0, 1.0, 1.0, 1.0]]))
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, start=np.zeros((2, 4)), scale=np.ones(3))
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, start=np.zeros((2, 4)), scale=np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, start=np.zeros((2, 4)), scale="iqr")
    with pytest.raises(ValueError):
        Dataset.kmeans(ds, 2, n_iters=-1)
    with pytest.raises(ValueError):
        Dataset.kmeans(_NoDevice(0, 4), 2)                      # an empty dataset
    with pytest.raises(ValueError):
        Dataset.kmeans_step(ds, np.zeros((17, 4)))
    with pytest.raises(ValueError):
        Dataset.kmeans_step(ds, np.zeros(4))
    with pytest.raises(ValueError):
        Dataset.kmeans_step(ds, np.full((2, 4), np.inf))
    with pytest.raises(ValueError):
        Dataset.kmeans_step(ds, np.zeros((2, 4)), np.full(4, np.nan))
    with pytest.raises(TypeError):
        Dataset.kmeans_step(ds, np.zeros((2, 4)), "std")
    import ppca_rs_amd as p

    for cls in (p.PPCAMix, p.FAMix):
        with pytest.raises(ValueError):
            cls.init(2, 1, _FakeDataset(50, 4), seed=1, method="spectral")


def _unpack(mix):
    return (np.array([m.isotropic_noise for m in mix.models]), np.stack([m.transform for m in mix.models]),
            np.stack([m.mean for m in mix.models]), mix.log_weights)


@pytest.mark.parametrize("case", TABLE, ids=lambda c: "%dx%d-k%d-m%d" % c[:4])
def test_kmeans_start_saves_mixture_iterations(oracle, case):
    """llk(k-means start + 3 EM iterations) > llk(PPCAMix.init(n_models, k, ds, seed) + 20), strictly, on the CPU: masked k-means of
    the restatement from u = default_rng(seed).random(n_models), PPCAModel.from_moments per cluster, oracle.mix_iterate.  Data:
    famix_restatement.synth(n, d, k, n_models, 1, masked, seed, separation).  Log-likelihood per row:

        (n, d, k, n_models, masked, seed, separation)   random + 0   random + 20   k-means + 0   k-means + 3
        (2000, 16, 2, 3, 0.3, 41, 3.0)                  -81.8813     -20.3173      -20.4607      -20.2827
        (3000, 24, 3, 4, 0.4, 42, 3.0)                  -69.86..     -29.8024      -26.2926      -26.1551
        (2500, 20, 2, 5, 0.5, 44, 3.0)                  -62.9346     -20.9512      -18.9895      -18.7677

    The second case has separation 3.0: at 2.0, (3000, 24, 3, 4, 0.4, 42, 2.0), the random start + 20 reaches -29.4688 and the k-means
    start + 3 only -29.7633 (the clusters overlap too much for a hard assignment to find them), so that case is not pinned.  K-means has
    local optima of its own: (1500, 12, 2, 3, 0.3, 43, 4.0) merges two clusters and loses, -18.2866 after 3 against -15.8091 after 20,
    which is why the defaults stay "random"."""
    import ppca_rs_amd as P

    n, d, k, nm, masked, seed, sep = case
    x, _, _, _ = FM.synth(n, d, k, nm, np.ones(d), masked, seed, separation=sep)
    rand = _unpack(P.PPCAMix.init(nm, k, _FakeDataset(n, d), seed=seed))
    for _ in range(20):
        rand = oracle.mix_iterate(x, *rand)
    km = KR.lloyd(x, None, nm, np.random.default_rng(seed).random(nm))
    assert np.all(km["history"][1:] <= km["history"][:-1] * (1.0 + 1e-12))
    start = _unpack(KR.ppca_mix_start(P, x, None, km["labels"], nm, k))
    l0 = oracle.mix_llks(x, *start).sum() / n
    for _ in range(3):
        start = oracle.mix_iterate(x, *start)
    la, lb = oracle.mix_llks(x, *start).sum() / n, oracle.mix_llks(x, *rand).sum() / n
    print(f"{case}: k-means + 0 {l0:.4f}, k-means + 3 {la:.4f}, random + 20 {lb:.4f} per row; smallest gap {km['min_gap']:.2e}")
    assert la > lb


def test_kmeans_start_of_the_fa_mixture():
    """Noise levels spread over 1e4: clustering in units of every column's standard deviation (scale="std"), FAModel.from_moments per
    cluster, the shared noise pooled; start + 3 ECM iterations of famix_restatement.iterate beat the random start + 10, and the start
    commutes with rescaling a column."""
    import ppca_rs_amd as P

    n, d, k, nm, masked, seed, sep = FA_CASE
    psi = fa_case_psi()
    assert psi.max() / psi.min() > 0.99e4
    x, _, _, _ = FM.synth(n, d, k, nm, psi, masked, seed, separation=sep)
    w = np.ones(n)
    r = P.PPCAMix.init(nm, k, _FakeDataset(n, d), seed=seed)
    rand = (np.ones(d), [m.transform for m in r.models], [m.mean for m in r.models], r.log_weights)
    for _ in range(10):
        rand = FM.iterate(x, w, *rand)[:4]
    u = np.random.default_rng(seed).random(nm)
    km = KR.lloyd(x, None, nm, u, scale=KR.column_std_scale(x))
    noise, cs, mus, lw = KR.fa_mix_start(P, x, None, km["labels"], nm, k)
    start = (noise, list(cs), list(mus), lw)
    l0 = FM.llks(x, *start).sum() / n
    for _ in range(3):
        start = FM.iterate(x, w, *start)[:4]
    la, lb = FM.llks(x, *start).sum() / n, FM.llks(x, *rand).sum() / n
    print(f"FA {FA_CASE}: k-means + 0 {l0:.4f}, k-means + 3 {la:.4f}, random + 10 {lb:.4f} per row; smallest gap {km['min_gap']:.2e}")
    assert la > lb
    # a column in other units: the same labels, the start rescaled with it
    a = np.ones(d)
    a[3] = 1e3
    km2 = KR.lloyd(x * a, None, nm, u, scale=KR.column_std_scale(x * a))
    assert np.array_equal(km2["labels"], km["labels"])
    noise2, cs2, mus2, lw2 = KR.fa_mix_start(P, x * a, None, km2["labels"], nm, k)
    for got, want in ((noise2, noise * a), (mus2, mus * a), (cs2, cs * a[None, :, None])):
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(lw2 - lw).max() <= 1e-12
