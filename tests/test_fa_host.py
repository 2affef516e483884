"""CPU-only: the factor-analysis surface (FAModel, FATrainer, Dataset.column_stats; the four C-ABI entry points behind them) is exported and
declared, ppca_fa_finalize_host -- the FA M-step on host buffers -- agrees with a dense numpy restatement in original units
(tests/fa_restatement.py), and FAModel's host-side logic (validation, serialisation, canonical form, whitening) holds."""
import ctypes as C
import io
import os
import pickle
import re

import numpy as np
import pytest

import fa_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("ppca_dataset_scale_columns", "ppca_dataset_fill_masked", "ppca_fa_finalize_host", "ppca_fa_em_step")


def test_fa_entry_points_exported(hiplib):
    from ppca_rs_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppca_hip.h")).read(), flags=re.S)
    for name in EXPORTS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert hiplib.ppca_abi_version() == 6


def test_fa_python_surface():
    import ppca_rs
    import ppca_rs_amd as p

    for name in ("FAModel", "FATrainer"):
        assert name in p.__all__ and hasattr(ppca_rs, name), name
    assert ppca_rs.FAModel is p.FAModel
    assert callable(getattr(p.Dataset, "column_stats", None))
    for meth in ("init", "from_ppca", "whitened", "to_canonical", "llk", "llks", "infer", "smooth", "extrapolate", "iterate",
                 "iterate_with_llk", "sample", "dump", "load"):
        assert callable(getattr(p.FAModel, meth, None)), meth
    for prop in ("noise", "transform", "mean", "output_size", "state_size", "n_parameters"):
        assert isinstance(getattr(p.FAModel, prop, None), property), prop
    assert callable(getattr(p.FATrainer, "train", None))


# --------------------------------------------------------------------------- ppca_fa_finalize_host against the restatement
def _packed_whitened_stats(x, w, psi, c, mu):
    """The packed statistics of include/ppca_hip.h (cross [d k] | S [d k'] lower-packed, e = a (a + 1) / 2 + b | U [d k] | sumx [d] |
    totals [d] | scalars [8]) of PPCAModel(1, C / psi, mu / psi) on the rows x / psi, and sq_j = sum w m (y_j - mean~_j)^2: numpy, row by row."""
    n, d = x.shape
    k = c.shape[1]
    kp = k * (k + 1) // 2
    a, mw, y = c / psi[:, None], mu / psi, x / psi
    cross, S, U = np.zeros((d, k)), np.zeros((d, kp)), np.zeros((d, k))
    sumx, tot, sq = np.zeros(d), np.zeros(d), np.zeros(d)
    lower = [(p, q) for p in range(k) for q in range(p + 1)]
    for i in range(n):
        o = np.isfinite(y[i])
        if not o.any():
            continue
        sigma = np.linalg.inv(np.eye(k) + a[o].T @ a[o])  # sigma = 1
        r = y[i, o] - mw[o]
        z = sigma @ (a[o].T @ r)
        P = np.outer(z, z) + sigma
        cross[o] += w[i] * np.outer(r, z)
        S[o] += w[i] * np.array([P[p, q] for p, q in lower])
        U[o] += w[i] * z
        sumx[o] += w[i] * r
        tot[o] += w[i]
        sq[o] += w[i] * r * r
    stats = np.concatenate([cross.ravel(), S.ravel(), U.ravel(), sumx, tot, np.zeros(8)])
    return stats, sq


def _finalize(hiplib, psi, c, mu, stats, sq, floor):
    from ppca_rs_amd import _lib

    d, k = c.shape
    assert stats.shape[0] == hiplib.ppca_stats_len(d, k)
    po, co, mo = np.empty(d), np.empty((d, k)), np.empty(d)
    _lib.check(hiplib.ppca_fa_finalize_host(d, k, _lib.ptr(psi), _lib.ptr(c), _lib.ptr(mu), _lib.ptr(stats), _lib.ptr(sq),
                                            _lib.ptr(floor), _lib.ptr(po), _lib.ptr(co), _lib.ptr(mo)))
    return po, co, mo


@pytest.fixture(scope="module")
def fa_case():
    """N = 400, d = 9, k = 3, 30 % masked, psi over 15x, weights, an all-masked row, an all-masked column; the model is a perturbed truth."""
    n, d, k = 400, 9, 3
    psi_true = np.geomspace(0.2, 3.0, d)
    x, c_true, mu_true = R.synth(n, d, k, psi_true, 0.3, 11)
    x[17] = np.nan
    x[:, 4] = np.nan
    rng = np.random.default_rng(12)
    w = rng.uniform(0.5, 2.0, n)
    psi = psi_true * rng.uniform(0.7, 1.4, d)
    c = c_true + 0.2 * psi_true[:, None] * rng.standard_normal((d, k))
    mu = mu_true + 0.3 * psi_true * rng.standard_normal(d)
    stats, sq = _packed_whitened_stats(x, w, psi, c, mu)
    return x, w, psi, c, mu, stats, sq


def _assert_model_close(got, want, rel=1e-10):
    (p1, c1, m1), (p0, c0, m0) = got, want
    assert np.all(np.abs(p1 - p0) <= rel * p0), np.abs(p1 / p0 - 1).max()
    assert np.abs(c1 - c0).max() <= rel * np.abs(c0).max()
    assert np.all(np.abs(m1 - m0) <= rel * np.maximum(np.abs(m0), p0))


def test_fa_finalize_host_matches_the_restatement(hiplib, fa_case):
    """fp64 host arithmetic on the same numbers on both sides: 1e-10 relative in psi, C and mean.  Weights, an all-masked row and an
    all-masked column are in the data; the all-masked column keeps its psi_j, c_j and mean_j."""
    x, w, psi, c, mu, stats, sq = fa_case
    got = _finalize(hiplib, psi, c, mu, stats, sq, None)
    want = R.iterate(x, w, psi, c, mu)
    _assert_model_close(got, want)
    assert got[0][4] == psi[4] and np.array_equal(got[1][4], c[4]) and got[2][4] == mu[4]
    moved = np.delete(np.arange(9), 4)
    assert np.all(np.abs(got[0][moved] / psi[moved] - 1) > 1e-6)  # (the step did something)


def test_fa_finalize_host_min_noise_binds_on_one_column(hiplib, fa_case):
    x, w, psi, c, mu, stats, sq = fa_case
    free = _finalize(hiplib, psi, c, mu, stats, sq, None)
    floor = np.zeros(9)
    floor[2] = 2.0 * free[0][2]
    got = _finalize(hiplib, psi, c, mu, stats, sq, floor)
    _assert_model_close(got, R.iterate(x, w, psi, c, mu, floor))
    assert got[0][2] == floor[2]
    keep = np.arange(9) != 2
    assert np.array_equal(got[0][keep], free[0][keep]) and np.array_equal(got[1], free[1]) and np.array_equal(got[2], free[2])


def test_fa_finalize_host_keeps_a_row_whose_system_is_singular(hiplib, fa_case):
    """S_3 = 0 with data present: the row is kept, and the mean and the noise follow from the full form with the kept row."""
    x, w, psi, c, mu, stats, sq = fa_case
    d, k = c.shape
    kp = k * (k + 1) // 2
    broken = stats.copy()
    broken[d * k + 3 * kp: d * k + 4 * kp] = 0.0
    got = _finalize(hiplib, psi, c, mu, broken, sq, None)
    assert np.array_equal(got[1][3], c[3])
    L_cross, L_U, L_sumx, L_tot = 0, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d
    a = c[3] / psi[3]
    tot = broken[L_tot + 3]
    delta = (broken[L_sumx + 3] - a @ broken[L_U + 3 * k: L_U + 4 * k]) / tot
    v = (sq[3] - 2.0 * a @ broken[L_cross + 3 * k: L_cross + 4 * k] - delta * delta * tot) / tot
    assert abs(got[2][3] - psi[3] * (mu[3] / psi[3] + delta)) <= 1e-10 * max(abs(mu[3]), psi[3])
    want_psi = psi[3] * np.sqrt(v) if v > 0 else psi[3]
    assert abs(got[0][3] - want_psi) <= 1e-10 * want_psi


def test_fa_finalize_host_rejects_bad_arguments(hiplib, fa_case):
    from ppca_rs_amd import PPCAError

    x, w, psi, c, mu, stats, sq = fa_case
    bad = psi.copy()
    bad[0] = 0.0
    with pytest.raises(PPCAError):
        _finalize(hiplib, bad, c, mu, stats, sq, None)


# --------------------------------------------------------------------------- FAModel host logic
def _model(d=6, k=2, seed=3):
    import ppca_rs_amd as p

    rng = np.random.default_rng(seed)
    return p.FAModel(rng.uniform(0.1, 4.0, d), rng.standard_normal((d, k)), rng.standard_normal(d))


def test_famodel_constructor_errors():
    import ppca_rs_amd as p

    c, mu = np.ones((4, 2)), np.zeros(4)
    with pytest.raises(ValueError):
        p.FAModel(np.ones(3), c, mu)  # wrong length
    with pytest.raises(ValueError):
        p.FAModel(1.0, c, mu)  # a scalar is the isotropic model, not this one
    with pytest.raises(ValueError):
        p.FAModel(np.ones((4, 1)), c, mu)
    for bad in (0.0, -1.0, np.nan, np.inf):
        n = np.ones(4)
        n[2] = bad
        with pytest.raises(ValueError):
            p.FAModel(n, c, mu)
    with pytest.raises(TypeError):
        p.FAModel(np.ones(4), np.ones(4), mu)  # transform must be 2-D, as PPCAModel
    with pytest.raises(ValueError):
        p.FAModel(np.ones(4), c, np.zeros(5))
    m = p.FAModel(np.ones(4), c, mu)
    assert (m.output_size, m.state_size, m.n_parameters) == (4, 2, 2 * 4 + 4 * 2)
    got = m.noise
    got[0] = 7.0
    assert m.noise[0] == 1.0  # the getters hand out copies


def test_famodel_dump_load_and_pickle_round_trip():
    import ppca_rs_amd as p

    m = _model()
    m = p.FAModel(m.noise, m.transform, np.where(m.mean > 0.5, -0.0, m.mean))  # (a sign bit that == does not see)
    fields = ("noise", "transform", "mean")
    for back in (p.FAModel.load(m.dump()), pickle.loads(pickle.dumps(m))):
        assert isinstance(back, p.FAModel)
        assert all(getattr(back, f).tobytes() == getattr(m, f).tobytes() and getattr(back, f).shape == getattr(m, f).shape for f in fields)
    z = np.load(io.BytesIO(m.dump()), allow_pickle=False)
    assert z.files == ["kind"] + list(fields) and str(z["kind"]) == "ppca_rs_amd.FAModel"
    assert all(z[f].dtype == np.float64 and z[f].tobytes() == getattr(m, f).tobytes() for f in fields)
    with pytest.raises(Exception) as err:
        p.FAModel.load(p.TPPCAModel(1.0, np.ones((3, 1)), np.zeros(3), 4.0).dump())  # another of the library's own containers
    assert type(err.value) is Exception and str(err.value) == "not an FAModel container: ppca_rs_amd.TPPCAModel"
    with pytest.raises(Exception):
        p.FAModel.load(p.PPCAModel(1.0, np.ones((3, 1)), np.zeros(3)).dump())  # another kind of container
    with pytest.raises(Exception):
        p.FAModel.load(b"not a container")


def test_famodel_to_canonical_keeps_covariance_noise_and_mean():
    import ppca_rs_amd as p

    m = _model(d=7, k=3)
    c = m.to_canonical()
    assert np.allclose(c.transform @ c.transform.T, m.transform @ m.transform.T, rtol=0, atol=1e-12 * np.abs(m.transform).max() ** 2)
    assert np.array_equal(c.noise, m.noise) and np.array_equal(c.mean, m.mean)
    want = p.PPCAModel(1.0, m.transform, m.mean).to_canonical().transform
    assert np.array_equal(c.transform, want)  # exactly PPCAModel's rotation
    norms = np.linalg.norm(c.transform, axis=0)
    assert np.all(np.diff(norms) <= 1e-12)


def test_famodel_from_ppca_and_whitened_by_hand():
    import ppca_rs_amd as p

    rng = np.random.default_rng(5)
    iso = p.PPCAModel(0.37, rng.standard_normal((5, 2)), rng.standard_normal(5))
    fa = p.FAModel.from_ppca(iso)
    assert np.array_equal(fa.noise, np.full(5, 0.37)) and np.array_equal(fa.transform, iso.transform) and np.array_equal(fa.mean, iso.mean)
    wh = fa.whitened()
    assert isinstance(wh, p.PPCAModel) and wh.isotropic_noise == 1.0
    assert np.array_equal(wh.transform, iso.transform / 0.37) and np.array_equal(wh.mean, iso.mean / 0.37)
    m = _model()
    wh = m.whitened()
    assert np.array_equal(wh.transform, m.transform / m.noise[:, None]) and np.array_equal(wh.mean, m.mean / m.noise)
