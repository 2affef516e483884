"""CPU-only: the pairwise-moments surface (ppca_dataset_pairwise_moments, PairwiseMoments, Dataset.pairwise_moments / covariance /
correlation, from_moments, method= / init=) is exported and declared; PairwiseMoments built from the numpy restatement
(tests/moments_restatement.py) reproduces pandas' pairwise covariance; and the spectral start PPCAModel.from_moments is the closed-form
maximum-likelihood model: a fixed point of the oracle's EM step on complete data."""
import inspect
import os
import re

import numpy as np
import pytest

import moments_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeDataset:
    """What PPCAModel.init(method="random") asks of a dataset, without a device."""

    def __init__(self, n, d, empty=()):
        self._n, self._dd, self._empty = n, d, list(empty)

    def __len__(self):
        return self._n

    def output_size(self):
        return self._dd

    def empty_dimensions(self):
        return self._empty


def _pm(x, w=None, center="mean"):
    from ppca_rs_amd import PairwiseMoments

    c = R.column_means(x, w) if isinstance(center, str) else (np.zeros(x.shape[1]) if center is None else center)
    return PairwiseMoments(c, *R.moments(x, w, c))


def test_moments_entry_point_exported(hiplib):
    from ppca_rs_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppca_hip.h")).read(), flags=re.S)
    name = "ppca_dataset_pairwise_moments"
    assert hasattr(hiplib, name)
    assert name in _lib.SIGNATURES
    assert re.search(r"\b%s\s*\(" % name, header)
    assert hiplib.ppca_abi_version() == 6


def test_moments_python_surface():
    import ppca_rs
    import ppca_rs_amd as p

    assert "PairwiseMoments" in p.__all__ and ppca_rs.PairwiseMoments is p.PairwiseMoments
    for meth in ("pairwise_moments", "covariance", "correlation"):
        assert callable(getattr(p.Dataset, meth, None)), meth
    for meth in ("covariance", "correlation", "__add__"):
        assert callable(getattr(p.PairwiseMoments, meth, None)), meth
    for prop in ("center", "sums", "counts", "cross"):
        assert isinstance(getattr(p.PairwiseMoments, prop, None), property), prop
    for cls in (p.PPCAModel, p.FAModel):
        assert callable(getattr(cls, "from_moments", None))
        sig = inspect.signature(cls.init)
        assert sig.parameters["method"].default == "random"
    for cls in (p.PPCATrainer, p.FATrainer):
        assert inspect.signature(cls.train).parameters["init"].default == "random"
    assert inspect.signature(p.Dataset.pairwise_moments).parameters["center"].default == "mean"
    assert inspect.signature(p.Dataset.pairwise_moments).parameters["cross"].default is False


def test_pairwise_covariance_is_pandas(oracle):
    import pandas

    x, _, _ = oracle.synth(500, 9, 3, 0.3, 11)
    x[:, 4] = np.nan          # an empty column: NaN row and column
    x[1:, 7] = np.nan         # one observation: counts <= ddof on its row and column
    want = pandas.DataFrame(x).cov().to_numpy()
    mom = _pm(x)
    got = mom.covariance("pairwise", ddof=1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).any() and np.isfinite(want).sum() > 40
    ok = np.isfinite(want)
    err = np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max()
    print("pairwise covariance against pandas: relative error", err)
    assert err < 1e-12
    # the centre does not matter to the pairwise form
    got0 = _pm(x, center=None).covariance("pairwise", ddof=1)
    assert np.abs(got0[ok] - want[ok]).max() / np.abs(want[ok]).max() < 1e-12
    # row blocks add up
    c = mom.center
    from ppca_rs_amd import PairwiseMoments

    a, b = PairwiseMoments(c, *R.moments(x[:200], None, c)), PairwiseMoments(c, *R.moments(x[200:], None, c))
    both = a + b
    for name in ("sums", "counts", "cross"):
        whole, parts = getattr(mom, name), getattr(both, name)
        assert np.abs(parts - whole).max() <= 1e-12 * np.abs(whole).max(), name
    assert np.array_equal(both.counts, mom.counts)
    with pytest.raises(ValueError):
        a + _pm(x[200:], center=None)
    with pytest.raises(ValueError):
        PairwiseMoments(c, mom.sums, mom.counts).covariance("pairwise")


def test_global_covariance_and_correlation(oracle):
    x, _, _ = oracle.synth(300, 6, 2, 0.3, 5)
    w = np.random.default_rng(3).uniform(0.5, 2.0, 300)
    mom = _pm(x, w)
    cov = mom.covariance()
    for j in range(6):
        for l in range(6):
            o = np.isfinite(x[:, j]) & np.isfinite(x[:, l])
            want = np.sum(w[o] * (x[o, j] - mom.center[j]) * (x[o, l] - mom.center[l])) / np.sum(w[o])
            assert abs(cov[j, l] - want) < 1e-12 * np.abs(cov).max()
    cor = mom.correlation()
    assert np.allclose(np.diag(cor), 1.0, atol=1e-14)
    assert np.allclose(cor, cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov))), atol=1e-14)
    assert np.all(np.isnan(mom.covariance(ddof=1e9)))


def test_closed_form_is_a_fixed_point_of_em(oracle):
    from ppca_rs_amd import PPCAModel

    x, _, _ = oracle.synth(2000, 12, 3, 0.0, 7)
    m = PPCAModel.from_moments(3, _pm(x))
    l0 = oracle.llk(x, m.isotropic_noise, m.transform, m.mean)
    s1, c1, m1 = oracle.iterate(x, m.isotropic_noise, m.transform, m.mean)
    l1 = oracle.llk(x, s1, c1, m1)
    print("closed form: llk", l0, "after one EM step", l1, "relative", abs(l1 - l0) / abs(l0), "sigma", m.isotropic_noise, s1)
    assert abs(l1 - l0) < 1e-10 * abs(l0)
    assert abs(s1 - m.isotropic_noise) < 1e-8 * s1
    # not vacuous: from the random start the same step moves the llk
    r = PPCAModel.init(3, _FakeDataset(2000, 12), seed=7, method="random")
    r0 = oracle.llk(x, r.isotropic_noise, r.transform, r.mean)
    r1 = oracle.llk(x, *oracle.iterate(x, r.isotropic_noise, r.transform, r.mean))
    assert abs(r1 - r0) > 1e-3 * abs(r0)
    # canonical: the signs are determined
    assert np.all(m.transform.sum(axis=0) >= 0.0)
    assert np.array_equal(m.to_canonical().transform.shape, (12, 3))


def test_from_moments_edge_cases(oracle):
    from ppca_rs_amd import FAModel, PPCAModel

    x, _, _ = oracle.synth(400, 7, 2, 0.3, 13)
    x[:, 2] = np.nan
    mom = _pm(x)
    m = PPCAModel.from_moments(2, mom)
    assert np.all(m.transform[2] == 0.0) and m.mean[2] == 0.0
    assert m.transform.shape == (7, 2) and np.isfinite(m.transform).all() and m.isotropic_noise > 0.0
    f = FAModel.from_moments(2, mom)
    assert np.all(f.transform[2] == 0.0) and f.mean[2] == 0.0 and f.noise[2] == 1.0
    # state_size 0: the isotropic model, sigma^2 = the mean variance of the live columns
    z = PPCAModel.from_moments(0, mom)
    live = [j for j in range(7) if j != 2]
    assert z.transform.shape == (7, 0)
    assert abs(z.isotropic_noise ** 2 - np.mean(np.diag(mom.covariance())[live])) < 1e-12
    # state_size >= d_live: every live direction taken, sigma at the floor, the columns past d_live zero
    for k in (6, 9):
        g = PPCAModel.from_moments(k, mom)
        cov = np.nan_to_num(mom.covariance())
        assert g.transform.shape == (7, k)
        assert abs(g.isotropic_noise ** 2 - 1e-8 * np.trace(cov) / 6) < 1e-18
        lam = np.linalg.eigvalsh(cov[np.ix_(live, live)])
        want = np.sort(np.maximum(lam - g.isotropic_noise ** 2, 0.0))[::-1]
        got = np.sort(np.sum(g.transform ** 2, axis=0))[::-1]
        assert np.allclose(got[:6], want, rtol=1e-9, atol=1e-12) and np.all(got[6:] < 1e-20)
    # no variance at all
    flat = np.tile(np.arange(4.0), (10, 1))
    q = PPCAModel.from_moments(2, _pm(flat))
    assert q.isotropic_noise == 1.0 and np.all(q.transform == 0.0) and np.array_equal(q.mean, np.arange(4.0))
    with pytest.raises(ValueError):
        PPCAModel.from_moments(-1, mom)


def test_fa_start_is_equivariant_under_column_scales(oracle):
    import fa_restatement as FR
    from ppca_rs_amd import FAModel

    rng = np.random.default_rng(32)
    psi = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), 10))
    x, _, _ = FR.synth(1000, 10, 2, psi, 0.4, 32)
    a = np.exp(rng.uniform(-3.0, 3.0, 10))
    f0, f1 = FAModel.from_moments(2, _pm(x)), FAModel.from_moments(2, _pm(x * a))
    worst = 0.0
    for got, want in ((f1.noise, f0.noise * a), (f1.mean, f0.mean * a), (f1.transform, f0.transform * a[:, None])):
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want).max(axis=-1, keepdims=True), 1e-300))))
    print("FA start under column scales: relative deviation", worst)
    assert worst < 1e-9


def test_random_init_is_unchanged():
    """method="random" (the default) is the draw of the reference's init as this library has always made it: column-major
    standard normals of default_rng(seed), empty columns zeroed, sigma 1, mean 0."""
    from ppca_rs_amd import FAModel, PPCAModel

    ds = _FakeDataset(50, 6, empty=[4])
    for seed in (0, 21, 12345):
        want = np.random.default_rng(seed).standard_normal(6 * 3).reshape((3, 6)).T.copy()
        want[4] = 0.0
        for m in (PPCAModel.init(3, ds, seed), PPCAModel.init(3, ds, seed=seed, method="random")):
            assert np.array_equal(m.transform, want) and m.isotropic_noise == 1.0 and np.array_equal(m.mean, np.zeros(6))
        f = FAModel.init(3, ds, seed=seed)
        assert np.array_equal(f.transform, want) and np.array_equal(f.noise, np.ones(6)) and np.array_equal(f.mean, np.zeros(6))
    for bad in (PPCAModel.init, FAModel.init):
        with pytest.raises(ValueError):
            bad(3, ds, seed=1, method="spectral")
        with pytest.raises(ValueError):
            bad(65, ds, method="pca")
        with pytest.raises(ValueError):
            bad(2, _FakeDataset(0, 6), method="pca")
