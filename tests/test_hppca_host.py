"""PPCA with a known precision per entry without a GPU: the C-ABI surface and the host-side M-step of the library against the row-by-row
restatement (tests/hppca_restatement.py), the restatement's own properties (its two forms agree; the log-likelihood never decreases;
its identities with the Gaussian model and with factor analysis; the heteroscedastic fit finds the subspace better than the Gaussian
one when the noise levels differ), and HPPCAModel's host-side surface."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

import fa_restatement as FA
import hppca_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_h_stats_len", "ppca_h_estep", "ppca_h_reconstruct", "ppca_h_finalize_host", "ppca_h_em_step")
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_and_surface(hiplib, P):
    from ppca_rs_amd import _lib

    header = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(hiplib, name), name
        decl = re.search(r"\bint(?:64_t)? %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert hiplib.ppca_abi_version() == 6 and re.search(r"#define\s+PPCA_ABI_VERSION\s+6\b", header)
    import ppca_rs

    assert ppca_rs.HPPCAModel is P.HPPCAModel and ppca_rs.HPPCATrainer is P.HPPCATrainer
    for name in ("isotropic_noise", "transform", "mean", "output_size", "state_size", "n_parameters", "init", "from_ppca", "gaussian",
                 "infer", "smooth", "extrapolate", "to_canonical", "llks", "llk", "iterate", "iterate_with_llk", "sample", "dump", "load"):
        assert hasattr(P.HPPCAModel, name), name
    assert hasattr(P.HPPCATrainer, "train")
    for d, k in ((1, 1), (17, 3), (1024, 16)):
        assert hiplib.ppca_h_stats_len(d, k) == d * (2 * k + k * (k + 1) // 2 + 4)


def test_restatement_forms_agree():
    x, p, w, (s, c, mu) = R.case(120, 40, 5, 6)
    x[60] = np.nan  # a row without an observed entry; row 61 has fewer observed entries than states
    keep = np.flatnonzero(R.observed(x[61], p[61]))[3:]
    x[61, keep] = np.nan
    a, b = R.estep(x, p, w, s, c, mu, dense=True), R.estep(x, p, w, s, c, mu, dense=False)
    assert a["m"][60] == 0 and 0 < a["m"][61] < 5
    for key in ("ell", "z", "Sigma"):
        err = (np.abs(a[key] - b[key]) / (1 + np.abs(a[key]))).max()
        print(key, "%.1e" % err)
        assert err <= 1e-9
    sa, sb, mag = R.packed_stats(a), R.packed_stats(b), R.packed_stats(a, "abs")
    err = (np.abs(sa - sb) / np.maximum(mag, 1e-300)).max()
    print("statistics %.1e of sum |terms|" % err)
    assert err <= 1e-9
    assert a["ell"][60] == 0 and not a["z"][60].any()


def test_finalize_host_against_the_restatement(hiplib):
    n, d, k = 400, 9, 3
    x, p, w, (s, c, mu) = R.case(n, d, k, 5)
    p[:, d // 3] = 0.0  # an all-empty column: T_j = 0
    e = R.estep(x, p, w, s, c, mu)
    stats = R.packed_stats(e)
    assert stats.shape[0] == hiplib.ppca_h_stats_len(d, k)
    s1, c1, m1 = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    assert hiplib.ppca_h_finalize_host(d, k, C.c_double(s), _p(c), _p(mu), _p(stats), C.byref(s1), _p(c1), _p(m1)) == 0
    ws, wc, wm = R.mstep(s, c, mu, e)
    errs = (abs(s1.value / ws - 1), np.abs(c1 - wc).max() / np.abs(wc).max(), np.abs(m1 - wm).max() / max(np.abs(wm).max(), ws))
    print("finalize: sigma %.1e C %.1e mean %.1e (bound 1e-12)" % errs)
    assert max(errs) <= 1e-12
    j = d // 3  # the all-empty column keeps its row of C and its mean
    assert e["T"][j] == 0 and np.array_equal(c1[j], c[j]) and m1[j] == mu[j]


def test_restatement_llk_never_decreases():
    x, p, w, _ = R.case(300, 10, 3, 7)
    rng = np.random.default_rng(8)
    m, prev = (1.0, rng.standard_normal((10, 3)), np.zeros(10)), -np.inf
    for it in range(20):
        m, llk = R.iterate(x, p, w, *m)
        assert llk >= prev - 1e-9 * abs(llk), (it, llk, prev)
        prev = llk
    print("llk %.6f sigma %.4f" % (prev, m[0]))


def test_unit_precisions_are_the_gaussian_model():
    from oracle import restate_numpy as G

    x, _, _, (s, c, mu) = R.case(80, 11, 3, 9)
    x[5] = np.nan
    e = R.estep(x, np.ones_like(x), None, s, c, mu, dense=False)
    want = G.llks(x, s, c, mu)
    assert (np.abs(e["ell"] - want) / (1 + np.abs(want))).max() <= 1e-10
    for i in range(len(x)):
        z, cov = G.infer_one(s, c, mu, x[i])
        assert np.abs(e["z"][i] - z).max() <= 1e-9 * (1 + np.abs(z).max()) and np.abs(e["Sigma"][i] - cov).max() <= 1e-9


def test_common_scale_of_sigma_and_precisions_cancels():
    x, p, w, (s, c, mu) = R.case(60, 9, 3, 10)
    a = 7.3
    for dense in (True, False):
        e0, e1 = R.estep(x, p, w, s, c, mu, dense=dense), R.estep(x, a * p, w, s * np.sqrt(a), c, mu, dense=dense)
        for key in ("ell", "z", "Sigma"):
            assert (np.abs(e0[key] - e1[key]) / (1 + np.abs(e0[key]))).max() <= 1e-10, (dense, key)


def test_column_precisions_are_factor_analysis():
    x, _, _, (_, c, mu) = R.case(70, 10, 3, 11)
    psi = np.random.default_rng(12).uniform(0.2, 2.0, 10)
    p = np.broadcast_to(1.0 / psi ** 2, x.shape).copy()
    for dense in (True, False):
        e = R.estep(x, p, None, 1.0, c, mu, dense=dense)
        want = FA.llks(x, psi, c, mu)
        assert (np.abs(e["ell"] - want) / (1 + np.abs(want))).max() <= 1e-10
        for i in (0, 7, 33):
            z, cov = FA.posterior(x[i], psi, c, mu)
            assert np.abs(e["z"][i] - z).max() <= 1e-9 * (1 + np.abs(z).max()) and np.abs(e["Sigma"][i] - cov).max() <= 1e-9


def hetero_angles():
    """The largest principal angles to the true subspace after HETERO["iters"] restated iterations from the same start: (with the true
    precisions, with every precision 1)."""
    x, p, c_true, c0 = R.hetero_case()
    out = []
    for prec in (p, np.ones_like(p)):
        m = (1.0, c0.copy(), np.zeros(x.shape[1]))
        for _ in range(R.HETERO["iters"]):
            m, _ = R.iterate(x, prec, None, *m)
        out.append(R.subspace_angle(m[1], c_true))
    return tuple(out)


def test_restatement_hetero_case():
    h, g = hetero_angles()
    print("true precisions: %.3f degrees from the true subspace; unit precisions: %.3f degrees" % (h, g))
    assert h < g
    # the figures the GPU test's margin (half the gap) is derived from
    assert abs(h - R.HETERO_ANGLES[0]) <= 1e-3 and abs(g - R.HETERO_ANGLES[1]) <= 1e-3


def test_argument_checks_without_a_gpu(hiplib, P):
    d, k = 6, 2
    c, mu, stats = np.zeros((1025, 17)), np.zeros(1025), np.zeros(8)
    s1 = C.c_double(0.0)
    for dd, kk in ((d, 17), (1025, k), (d, 0), (0, k)):
        rc = hiplib.ppca_h_finalize_host(dd, kk, C.c_double(1.0), _p(c), _p(mu), _p(stats), C.byref(s1), _p(c), _p(mu))
        assert rc == UNSUPPORTED, (dd, kk, rc)
        assert b"state sizes 1 .. 16" in hiplib.ppca_last_error()
        rc = hiplib.ppca_h_em_step(None, None, None, dd, kk, C.c_double(1.0), _p(c), _p(mu), C.byref(s1), _p(c), _p(mu), None)
        assert rc == UNSUPPORTED, (dd, kk, rc)
    assert hiplib.ppca_h_em_step(None, None, None, d, k, C.c_double(1.0), _p(c), _p(mu), C.byref(s1), _p(c), _p(mu), None) == INVALID
    assert hiplib.ppca_h_finalize_host(d, k, C.c_double(-1.0), _p(c), _p(mu), _p(stats), C.byref(s1), _p(c), _p(mu)) == INVALID
    assert hiplib.ppca_h_estep(None, None, None, None, None, None, None, None, None) == INVALID
    with pytest.raises(ValueError, match="state sizes 1 .. 16"):
        P.HPPCAModel(0.5, np.zeros((20, 17)), np.zeros(20))
    with pytest.raises(ValueError, match="state sizes 1 .. 16"):
        P.HPPCAModel(0.5, np.zeros((7, 0)), np.zeros(7))
    with pytest.raises(ValueError, match="output sizes 1 .. 1024"):
        P.HPPCAModel(0.5, np.zeros((1025, 2)), np.zeros(1025))
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            P.HPPCAModel(bad, np.zeros((7, 2)), np.zeros(7))
    m = P.HPPCAModel(0.5, np.ones((7, 2)), np.zeros(7))
    with pytest.raises(ValueError, match=r"precisions must be \(N, 7\)"):  # a shape mismatch
        m.sample(np.ones((5, 6)))
    with pytest.raises(ValueError, match="negative or \\+inf"):
        m.sample(np.full((5, 7), -1.0))


def test_model_host_surface(P):
    rng = np.random.default_rng(1)
    c, mu = rng.standard_normal((7, 3)), rng.standard_normal(7)
    m = P.HPPCAModel(0.5, c, mu)
    assert (m.isotropic_noise, m.output_size, m.state_size) == (0.5, 7, 3)
    assert np.array_equal(m.transform, c) and np.array_equal(m.mean, mu)
    assert m.n_parameters == P.PPCAModel(0.5, c, mu).n_parameters == 1 + 21 + 7
    assert "HPPCAModel(" in repr(m)
    g = m.gaussian()
    assert isinstance(g, P.PPCAModel) and g.isotropic_noise == 0.5 and np.array_equal(g.transform, c) and np.array_equal(g.mean, mu)
    assert np.array_equal(P.HPPCAModel.from_ppca(g).transform, c)
    can = m.to_canonical()
    assert can.isotropic_noise == 0.5 and np.array_equal(can.mean, mu) and np.array_equal(can.transform, g.to_canonical().transform)
    for back in (P.HPPCAModel.load(m.dump()), pickle.loads(pickle.dumps(m))):
        assert isinstance(back, P.HPPCAModel) and back.isotropic_noise == 0.5
        assert back.transform.tobytes() == c.tobytes() and back.mean.tobytes() == mu.tobytes()
    with pytest.raises(Exception) as err:
        P.HPPCAModel.load(P.FAModel(np.ones(7), c, mu).dump())
    assert type(err.value) is Exception and str(err.value) == "not a HPPCAModel container: ppca_rs_amd.FAModel"
