"""Student-t PPCA on row-compressed data without a GPU: the C-ABI surface, the host M-step fed with statistics
of the scaled-dataset form on the sparse cases, the row_compressed flag of TPPCAModel, and every refusal that must come before a
device is touched."""
import ctypes as C
import io
import os
import pickle
import re

import numpy as np
import pytest

import sparse_t_cases as T
import tppca_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_t_sparse_estep", "ppca_t_sparse_em_step")


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def test_symbols_and_surface(hiplib, P):
    from ppca_rs_amd import _lib

    header = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert hiplib.ppca_abi_version() == 6 and re.search(r"#define\s+PPCA_ABI_VERSION\s+6\b", header)
    assert "ppca_sparse_robust.hip" in __import__("ppca_rs_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("predict", "row_compressed"):
        assert hasattr(P.TPPCAModel, name), name


@pytest.mark.parametrize("n,d,k", [(64, 9, 3), (150, 300, 11)], ids=["64x9x3", "150x300x11"])
def test_finalize_host_on_the_scaled_form(hiplib, n, d, k):
    """ppca_t_finalize_host fed with the statistics the sparse step forms (the EM statistics of PPCAModel(sigma, C, 0) on
    Y = sqrt(u) (x - mean), and the k + 3 column sums) against tppca_restatement.mstep in the direct form, at the bound of
    tests/test_tppca_host.py::test_finalize_host_against_the_restatement (1e-10).  Column 5 has no entry and keeps its row of C and its
    mean; column 3 has the one entry of row 0."""
    nu = T.NU
    x, w, (s, c, mu) = T.case(n, d, k)
    assert not np.isfinite(x[:, 5]).any() and np.isfinite(x[:, 3]).sum() == 1 and (w == 0).sum() == 1
    e = T.want(n, d, k, nu)
    stats = T.packed_stats_of_scaled(x, w, s, c, mu, e["u"])
    assert stats.shape[0] == hiplib.ppca_stats_len(d, k)
    sums = np.concatenate([e["V"].ravel(), e["A"], e["T"], e["sq"]])
    s1, c1, m1 = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert hiplib.ppca_t_finalize_host(d, k, C.c_double(s), p(c), p(mu), p(stats), p(sums), C.byref(s1), p(c1), p(m1)) == 0
    ws, wc, wm = R.mstep(s, c, mu, e)
    errs = (abs(s1.value / ws - 1), np.abs(c1 - wc).max() / np.abs(wc).max(), np.abs(m1 - wm).max() / max(np.abs(wm).max(), ws))
    print("finalize %dx%dx%d: sigma %.1e C %.1e mean %.1e (bound 1e-10)" % ((n, d, k) + errs))
    assert max(errs) <= 1e-10
    assert np.array_equal(c1[5], c[5]) and m1[5] == mu[5]


def test_the_row_compressed_flag(P):
    d, k = 1500, 2
    c, mu = np.random.default_rng(0).standard_normal((d, k)), np.zeros(d)
    with pytest.raises(ValueError, match=r"covers state sizes 1 \.\. 16 and output sizes 1 \.\. 1024 \(got k=2, d=1500\)"):
        P.TPPCAModel(0.5, c, mu, 4.0)
    with pytest.raises(ValueError, match="covers state sizes"):
        P.TPPCAModel(0.5, np.zeros((1025, 2)), np.zeros(1025), 4.0)
    with pytest.raises(TypeError):
        P.TPPCAModel(0.5, c, mu, 4.0, None, False, True)  # keyword-only
    m = P.TPPCAModel(0.5, c, mu, 4.0, row_compressed=True)
    assert m.row_compressed and m.output_size == d and not P.TPPCAModel(0.5, c[:9], mu[:9], 4.0).row_compressed
    with pytest.raises(ValueError, match="covers state sizes"):  # the state-size limit stays
        P.TPPCAModel(0.5, np.zeros((d, 17)), mu, 4.0, row_compressed=True)
    # init on a SparseDataset sets it; on a Dataset-shaped argument it stays off
    x, w, _ = T.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    a = P.TPPCAModel.init(3, sp, seed=5, dof=3.0)
    assert a.row_compressed and a.dof == 3.0 and sp._handle is None
    g = P.PPCAModel.init(3, sp, seed=5)
    assert np.array_equal(a.transform, g.transform) and not a.transform[5].any()
    with pytest.raises(ValueError, match="method='pca' is not available on a SparseDataset"):
        P.TPPCAModel.init(3, sp, method="pca")
    with pytest.raises(ValueError, match="method='pca' is not available on a SparseDataset"):
        P.TPPCATrainer(sp).train(state_size=3, init="pca", quiet=True)
    # from_ppca and to_canonical carry it
    assert P.TPPCAModel.from_ppca(P.PPCAModel(0.5, c, mu), 4.0, row_compressed=True).row_compressed
    assert not P.TPPCAModel.from_ppca(P.PPCAModel(0.5, c[:9], mu[:9]), 4.0).row_compressed
    can = m.to_canonical()
    assert can.row_compressed and can.output_size == d
    # dump / load / pickle
    back = P.TPPCAModel.load(m.dump())
    assert back.row_compressed and np.array_equal(back.transform, c) and back.dof == 4.0
    pk = pickle.loads(pickle.dumps(m))
    assert pk.row_compressed and pk.output_size == d and np.array_equal(pk.transform, c) and pk.isotropic_noise == 0.5
    assert not pickle.loads(pickle.dumps(P.TPPCAModel(0.5, c[:9], mu[:9], 4.0))).row_compressed
    # a dump written before the flag existed loads with the flag off
    buf = io.BytesIO()
    np.savez(buf, kind="ppca_rs_amd.TPPCAModel", isotropic_noise=0.5, transform=c[:9], mean=mu[:9], dof=4.0, estimated_dof=True)
    old = P.TPPCAModel.load(buf.getvalue())
    assert not old.row_compressed and old.n_parameters == P.PPCAModel(0.5, c[:9], mu[:9]).n_parameters + 1


def test_refusals_come_before_any_device(P):
    x, w, (s, c, mu) = T.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.TPPCAModel(s, c, mu, 4.0)
    train, held = sp.holdout(0.3, 1)
    with pytest.raises(TypeError, match="PPCAModel.heldout_score") as err:
        model.score_heldout(train, held)
    assert "score_heldout" in str(err.value) and "not built on row-compressed data" in str(err.value)
    with pytest.raises(TypeError, match="PPCAModel.heldout_score") as err:
        P.TPPCATrainer(sp).select_state_size([2, 3], seed=1, n_iters=1)
    assert "select_state_size" in str(err.value) and "not built on row-compressed data" in str(err.value)
    with pytest.raises(TypeError, match="TPPCAModel"):  # the package-level function keeps its own refusal
        P.heldout_score(model, train, held)
    other = P.TPPCAModel(s, np.ones((10, 3)), np.zeros(10), 4.0)  # another d
    for call in (other.llks, other.llk, other.row_weights, other.mahalanobis, other.iterate, other.iterate_with_llk):
        with pytest.raises(ValueError, match="output size"):
            call(sp)
    empty = P.SparseDataset([0], [], [], 9)
    with pytest.raises(ValueError, match="empty"):
        model.iterate(empty)
    with pytest.raises(ValueError, match="empty"):
        model.iterate_with_llk(empty, estimate_dof=True)
    with pytest.raises(ValueError, match="covers state sizes"):  # k = 17 never becomes a model
        P.TPPCAModel(s, np.ones((9, 17)), mu, 4.0, row_compressed=True)
    with pytest.raises(ValueError, match="state_size"):
        P.TPPCAModel.init(0, sp)
    with pytest.raises(TypeError):
        model.smooth(sp)
    with pytest.raises(TypeError):
        model.extrapolate(sp)
    for ds in (sp, train, held, empty):
        assert ds._handle is None


def test_the_wording_of_the_dense_only_error(P):
    x, w, _ = T.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    with pytest.raises(TypeError) as err:
        sp._h
    for text in ("not available on a SparseDataset (DESIGN.md section 7)", "predict", "PPCAMix.llk / llks / infer_cluster",
                 "FAModel.llk / llks / infer", "FATrainer", "TPPCAModel.llk / llks / row_weights / mahalanobis", "TPPCATrainer.train"):
        assert text in str(err.value), text
    assert sp._handle is None
