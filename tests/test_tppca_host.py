"""Student-t PPCA without a GPU: the C-ABI surface, the host-side tables and M-step of the library against the row-by-row restatement
(tests/tppca_restatement.py), the restatement's own properties (its two forms of delta and ln det agree; the t log-likelihood never
decreases; the t fit survives contamination that the Gaussian limit does not), and TPPCAModel's host-side surface."""
import ctypes as C
import io
import math
import os
import pickle
import re

import numpy as np
import pytest

import tppca_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_t_tables_host", "ppca_t_estep", "ppca_t_finalize_host", "ppca_t_em_step")


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def test_symbols_and_surface(hiplib, P):
    from ppca_rs_amd import _lib

    header = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(hiplib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert hiplib.ppca_abi_version() == 6 and re.search(r"#define\s+PPCA_ABI_VERSION\s+6\b", header)
    import ppca_rs

    assert ppca_rs.TPPCAModel is P.TPPCAModel and ppca_rs.TPPCATrainer is P.TPPCATrainer
    for name in ("isotropic_noise", "transform", "mean", "dof", "output_size", "state_size", "n_parameters", "init", "from_ppca", "gaussian",
                 "infer", "smooth", "extrapolate", "to_canonical", "llks", "llk", "row_weights", "mahalanobis", "iterate",
                 "iterate_with_llk", "sample", "dump", "load"):
        assert hasattr(P.TPPCAModel, name), name
    assert hasattr(P.TPPCATrainer, "train")


def _digamma_reference(x):
    try:
        from scipy.special import digamma

        return float(digamma(x)), 1e-13
    except ImportError:
        # central differences of ln Gamma at h and h / 2, Richardson-extrapolated (error O(h^4)); the rounding of lgamma / h decides
        def cd(h):
            return (math.lgamma(x + h) - math.lgamma(x - h)) / (2.0 * h)
        h = 1e-3 * max(x, 1.0)
        return (4.0 * cd(0.5 * h) - cd(h)) / 3.0, 1e-8


@pytest.mark.parametrize("nu", [0.5, 4.0, 1e3])
def test_tables(hiplib, nu):
    d = 40
    lg, g = np.empty(d + 1), np.empty(d + 1)
    assert hiplib.ppca_t_tables_host(d, C.c_double(nu), lg.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)) == 0
    worst_lg = worst_g = 0.0
    for m in range(d + 1):
        want = math.lgamma(0.5 * (nu + m)) - math.lgamma(0.5 * nu) - 0.5 * m * math.log(nu * math.pi)
        terms = abs(math.lgamma(0.5 * (nu + m))) + abs(math.lgamma(0.5 * nu)) + abs(0.5 * m * math.log(nu * math.pi)) + 1.0
        worst_lg = max(worst_lg, abs(lg[m] - want) / terms)
        psi, tol = _digamma_reference(0.5 * (nu + m))
        worst_g = max(worst_g, abs(g[m] - (psi - math.log(0.5 * (nu + m)))) / (abs(psi) + 1.0) / tol)
    print(f"nu={nu}: lg {worst_lg:.2e} (bound 1e-14 of the terms), g {worst_g:.2e} of its bound")
    assert worst_lg <= 1e-14 and worst_g <= 1.0
    assert lg[0] == 0.0
    # the library's large-nu branch (Stirling's series term by term) against mpmath-free arithmetic: continuity across the switch
    for nu2 in (1.9999e4, 2.0001e4):
        hiplib.ppca_t_tables_host(d, C.c_double(nu2), lg.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p))
        want = math.lgamma(0.5 * (nu2 + d)) - math.lgamma(0.5 * nu2) - 0.5 * d * math.log(nu2 * math.pi)
        assert abs(lg[d] - want) <= 1e-10  # (lgamma's own cancellation at 1e5 |ln Gamma| is ~1e-11)
    assert hiplib.ppca_t_tables_host(d, C.c_double(0.0), lg.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)) != 0


def _packed_stats_of_scaled(x, w, sigma, c, mu, u):
    """The packed statistics (include/ppca_hip.h) of PPCAModel(sigma, C, 0) on y = sqrt(u) (x - mean), in numpy"""
    n, d = x.shape
    k = c.shape[1]
    kp = k * (k + 1) // 2
    y = np.sqrt(u)[:, None] * (x - mu)
    cross, S, totals = np.zeros((d, k)), np.zeros((d, kp)), np.zeros(d)
    for i in range(n):
        o = np.isfinite(y[i])
        if not o.any():
            continue
        co = c[o]
        M = sigma ** 2 * np.eye(k) + co.T @ co
        z = np.linalg.solve(M, co.T @ y[i, o])
        P = sigma ** 2 * np.linalg.inv(M) + np.outer(z, z)
        cross[o] += w[i] * np.outer(y[i, o], z)
        S[o] += w[i] * np.array([P[a, b] for a in range(k) for b in range(a + 1)])
        totals[o] += w[i]
    return np.concatenate([cross.ravel(), S.ravel(), np.zeros(d * k), np.zeros(d), totals, np.zeros(8)])


def test_finalize_host_against_the_restatement(hiplib):
    n, d, k, nu = 400, 9, 3, 4.0
    x, w, (s, c, mu) = R.masked_case(n, d, k, 5)
    e = R.estep(x, w, s, c, mu, nu)
    stats = _packed_stats_of_scaled(x, w, s, c, mu, e["u"])
    assert stats.shape[0] == hiplib.ppca_stats_len(d, k)
    sums = np.concatenate([e["V"].ravel(), e["A"], e["T"], e["sq"]])
    s1, c1, m1 = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert hiplib.ppca_t_finalize_host(d, k, C.c_double(s), p(c), p(mu), p(stats), p(sums), C.byref(s1), p(c1), p(m1)) == 0
    ws, wc, wm = R.mstep(s, c, mu, e)
    errs = (abs(s1.value / ws - 1), np.abs(c1 - wc).max() / np.abs(wc).max(), np.abs(m1 - wm).max() / max(np.abs(wm).max(), ws))
    print("finalize: sigma %.1e C %.1e mean %.1e (bound 1e-10)" % errs)
    assert max(errs) <= 1e-10
    j = d // 3  # the all-masked column keeps its row of C and its mean
    assert np.array_equal(c1[j], c[j]) and m1[j] == mu[j]


def test_restatement_forms_agree():
    x, w, (s, c, mu) = R.masked_case(120, 40, 5, 6)
    a, b = R.estep(x, w, s, c, mu, 3.0, dense=True), R.estep(x, w, s, c, mu, 3.0, dense=False)
    for key in ("delta", "u", "ell"):
        err = (np.abs(a[key] - b[key]) / (1 + np.abs(a[key]))).max()
        print(key, "%.1e" % err)
        assert err <= 1e-11
    assert a["delta"][60] == 0 and a["u"][60] == 1 and a["ell"][60] == 0  # the all-masked row


@pytest.mark.parametrize("estimate", [False, True], ids=["nu-fixed", "nu-estimated"])
def test_restatement_llk_never_decreases(estimate):
    x, w, _ = R.masked_case(300, 10, 3, 7)
    rng = np.random.default_rng(8)
    m, prev = (1.0, rng.standard_normal((10, 3)), np.zeros(10), 4.0), -np.inf
    for it in range(30):
        m, llk = R.iterate(x, w, *m, estimate_dof=estimate)
        assert llk >= prev - 1e-9 * abs(llk), (it, llk, prev)
        prev = llk
    print("llk %.6f nu %.3f" % (prev, m[3]))


def test_restatement_contaminated_case():
    x, c, bad, c0 = R.contaminated_start()
    angles = {}
    for nu in (4.0, 1e12):
        m = (1.0, c0.copy(), np.zeros(x.shape[1]), nu)
        for _ in range(30):
            m, _ = R.iterate(x, None, *m)
        angles[nu] = R.subspace_angle(m[1], c)
        print("nu=%g: %.2f degrees from the true subspace, sigma %.3f (true 0.5)" % (nu, angles[nu], m[0]))
    assert angles[4.0] < 5.0 and angles[1e12] > 20.0


def test_model_host_surface(P):
    rng = np.random.default_rng(1)
    c, mu = rng.standard_normal((7, 3)), rng.standard_normal(7)
    m = P.TPPCAModel(0.5, c, mu, 4.0)
    assert (m.isotropic_noise, m.dof, m.output_size, m.state_size) == (0.5, 4.0, 7, 3)
    assert np.array_equal(m.transform, c) and np.array_equal(m.mean, mu)
    assert m.n_parameters == P.PPCAModel(0.5, c, mu).n_parameters == 1 + 21 + 7
    assert "TPPCAModel(" in repr(m) and "dof=4.0" in repr(m)
    g = m.gaussian()
    assert isinstance(g, P.PPCAModel) and g.isotropic_noise == 0.5 and np.array_equal(g.transform, c) and np.array_equal(g.mean, mu)
    f = P.TPPCAModel.from_ppca(g, 7.5)
    assert f.dof == 7.5 and np.array_equal(f.transform, c)
    can = m.to_canonical()
    assert can.dof == 4.0 and can.isotropic_noise == 0.5 and np.array_equal(can.mean, mu)
    assert np.allclose(can.transform @ can.transform.T, c @ c.T, atol=1e-12)
    assert np.array_equal(can.transform, g.to_canonical().transform)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            P.TPPCAModel(0.5, c, mu, bad)
    with pytest.raises(ValueError, match="state sizes 1 .. 16"):
        P.TPPCAModel(0.5, np.zeros((7, 0)), mu, 4.0)
    with pytest.raises(ValueError, match="state sizes 1 .. 16"):
        P.TPPCAModel(0.5, np.zeros((20, 17)), np.zeros(20), 4.0)
    with pytest.raises(ValueError, match="output sizes 1 .. 1024"):
        P.TPPCAModel(0.5, np.zeros((1025, 2)), np.zeros(1025), 4.0)
    with pytest.raises(ValueError):
        P.TPPCAModel(0.0, c, mu, 4.0)
    for back in (P.TPPCAModel.load(m.dump()), pickle.loads(pickle.dumps(m))):
        assert back.dof == 4.0 and back.isotropic_noise == 0.5 and np.array_equal(back.transform, c) and np.array_equal(back.mean, mu)
        assert back.n_parameters == m.n_parameters
    mu0 = np.where(mu > 0.5, -0.0, mu)  # (a sign bit that == does not see)
    e = P.TPPCAModel(0.1 + 0.2, c, mu0, 1.0 / 3.0, _estimated_dof=True)
    for back in (P.TPPCAModel.load(e.dump()), pickle.loads(pickle.dumps(e))):
        assert isinstance(back, P.TPPCAModel) and back._estimated is True and (back.dof, back.isotropic_noise) == (1.0 / 3.0, 0.1 + 0.2)
        assert back.transform.tobytes() == c.tobytes() and back.mean.tobytes() == mu0.tobytes() and back.transform.shape == c.shape
    assert pickle.loads(pickle.dumps(m))._estimated is False
    z = np.load(io.BytesIO(e.dump()), allow_pickle=False)
    assert z.files == ["kind", "isotropic_noise", "transform", "mean", "dof", "estimated_dof"] and str(z["kind"]) == "ppca_rs_amd.TPPCAModel"
    assert all(z[f].dtype == np.float64 for f in ("isotropic_noise", "transform", "mean", "dof")) and z["estimated_dof"].dtype == np.bool_
    assert z["transform"].tobytes() == c.tobytes() and z["mean"].tobytes() == mu0.tobytes() and float(z["dof"]) == 1.0 / 3.0
    with pytest.raises(Exception):
        P.TPPCAModel.load(P.PPCAModel(0.5, c, mu).dump())
    with pytest.raises(Exception) as err:
        P.TPPCAModel.load(P.FAModel(np.ones(7), c, mu).dump())  # another of the library's own containers
    assert type(err.value) is Exception and str(err.value) == "not a TPPCAModel container: ppca_rs_amd.FAModel"


def test_dof_root_matches_the_restatement(P):
    from ppca_rs_amd.api import _t_dof_root

    for q in (-1.02, -1.2, -2.0, -1.0000001, -0.5, -50.0):
        a, b = _t_dof_root(q), R.dof_root(q)
        assert abs(a - b) <= 1e-9 * b, (q, a, b)
    assert R.dof_root(-0.5) == 1e4 and R.dof_root(-50.0) == 1e4  # no sign change: the upper end
