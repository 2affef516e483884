"""PPCA with a known precision per entry on row-compressed data without a GPU: the C-ABI surface, every
refusal that must come before a device is touched, the row_compressed flag of HPPCAModel, SparseDataset.with_values and the aligned
split of data and precisions, the inputs of the GPU tests, and the case that justifies the feature recomputed from the restatement."""
import ctypes as C
import io
import os
import pickle
import re

import numpy as np
import pytest

import hppca_restatement as R
import sparse_h_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_h_sparse_precisions", "ppca_h_sparse_estep", "ppca_h_sparse_em_step", "ppca_h_sparse_predict")
HANDLES = ("ppca_ctx", "ppca_dataset", "ppca_sparse", "ppca_comm")
INVALID = -1


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def test_symbols_and_surface(hiplib, P):
    from ppca_rs_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppca_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert len(params) == len(_lib.SIGNATURES[name][1]), name
        # tests/test_sparse_host.py pins the ppca_sparse_* symbols; tests/test_recycled_memory_host.py claims every entry point that
        # leads with a handle for its inventory: these lead with the model or the host arrays
        assert not name.startswith("ppca_sparse_")
        assert not any(re.search(r"\b%s\b" % h, params[0]) for h in HANDLES), (name, params[0])
    assert hiplib.ppca_abi_version() == 6 and re.search(r"#define\s+PPCA_ABI_VERSION\s+6\b", header)
    assert "ppca_sparse_hetero.hip" in __import__("ppca_rs_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("predict", "row_compressed"):
        assert hasattr(P.HPPCAModel, name), name
    assert hasattr(P.SparseDataset, "with_values")
    # the null checks of the C entry points need no device
    assert hiplib.ppca_h_sparse_precisions(None, None, None, None) == INVALID
    assert hiplib.ppca_h_sparse_estep(None, None, None, None, None, None, None, None, None) == INVALID
    one = np.ones(1)
    p = one.ctypes.data_as(C.c_void_p)
    assert hiplib.ppca_h_sparse_estep(None, None, None, None, p, None, None, None, None) == INVALID
    assert hiplib.ppca_h_sparse_em_step(1, 1, C.c_double(1.0), p, p, None, None, None, None, None, None, None) == INVALID
    assert hiplib.ppca_h_sparse_predict(None, None, None, None, None, None, None, None) == INVALID


def _case(P, n=64, d=9, k=3):
    x, p, w, (s, c, mu), pv = H.case(n, d, k)
    return P.SparseDataset.from_dense(x, w), pv, P.HPPCAModel(s, c, mu)


def test_refusals_come_before_any_device(P):
    sp, pv, model = _case(P)
    q = (sp.csr()[0], sp.csr()[1])
    passes = [lambda p: model.llk(sp, p), lambda p: model.llks(sp, p), lambda p: model.infer(sp, p), lambda p: model.iterate(sp, p),
              lambda p: model.iterate_with_llk(sp, p), lambda p: model.predict(sp, p, q),
              lambda p: P.HPPCATrainer(sp, p).train(state_size=3, n_iters=1, seed=1)]
    # a wrong length
    for call in passes:
        with pytest.raises(ValueError, match="one precision per stored entry"):
            call(pv[:-1])
        with pytest.raises(ValueError, match="one precision per stored entry"):
            call(np.ones((len(sp), 9)))
    # a differing pattern: the train part of a split, another column count
    other = sp.holdout(0.3, 1)[0]
    wide = P.SparseDataset(sp.csr()[0], sp.csr()[1], pv, 10)
    for call in passes:
        for bad in (other, wide):
            with pytest.raises(ValueError, match="differ in pattern"):
                call(bad)
    # a bad precision: on this data there is no masking precision
    for v in (0.0, -1.0, np.nan, np.inf, -np.inf):
        bad = pv.copy()
        bad[len(bad) // 2] = v
        for call in passes:
            with pytest.raises(ValueError, match="finite and > 0"):
                call(bad)
    with pytest.raises(ValueError, match="finite and > 0"):
        model.llks(sp, sp.with_values(np.where(np.arange(sp.nnz) == 3, 0.0, pv)))
    # a dataset of another output size, an empty one
    small = P.HPPCAModel(0.5, np.ones((10, 3)), np.zeros(10))
    for call in (small.llk, small.llks, small.infer, small.iterate, small.iterate_with_llk):
        with pytest.raises(ValueError, match="output size"):
            call(sp, pv)
    with pytest.raises(ValueError, match="output size"):
        small.predict(sp, pv, q)
    empty = P.SparseDataset([0], [], [], 9)
    for call in (model.llk, model.llks, model.infer, model.iterate, model.iterate_with_llk):
        with pytest.raises(ValueError, match="empty"):
            call(empty, np.zeros(0))
    with pytest.raises(ValueError, match="empty"):
        model.predict(empty, np.zeros(0), ([0], []))
    # what is not built: TypeError, naming what exists
    with pytest.raises(TypeError, match="HPPCAModel.predict"):
        model.smooth(sp, pv)
    with pytest.raises(TypeError, match="HPPCAModel.predict"):
        model.extrapolate(sp, pv)
    train, held = sp.holdout(0.3, 1)
    with pytest.raises(TypeError, match="HPPCATrainer.train") as err:
        model.score_heldout(train, held, pv)
    assert "score_heldout" in str(err.value) and "not built on row-compressed data" in str(err.value)
    with pytest.raises(TypeError, match="HPPCATrainer.train") as err:
        P.HPPCATrainer(sp, pv).select_state_size([2, 3], seed=1, n_iters=1)
    assert "select_state_size" in str(err.value) and "PPCAModel.heldout_score" in str(err.value)
    # unchanged, because existing tests pin them
    with pytest.raises(ValueError, match="precisions are not available with a SparseDataset"):
        P.cross_validate(sp, lambda tr, pr: None, precisions=pv)
    with pytest.raises(TypeError, match="HPPCAModel does not score a SparseDataset"):
        P.heldout_score(model, train, held, pv)
    # init
    with pytest.raises(ValueError, match="method='pca' is not available on a SparseDataset"):
        P.HPPCAModel.init(3, sp, method="pca")
    with pytest.raises(ValueError, match="method='pca' is not available on a SparseDataset"):
        P.HPPCATrainer(sp, pv).train(state_size=3, init="pca")
    with pytest.raises(ValueError, match="covers state sizes"):  # k = 17 never becomes a model
        P.HPPCAModel(0.5, np.ones((9, 17)), np.zeros(9), row_compressed=True)
    for ds in (sp, other, wide, empty, train, held):
        assert ds._handle is None


def test_the_wording_of_the_dense_only_error(P):
    sp, _, _ = _case(P)
    with pytest.raises(TypeError) as err:
        sp._h
    for text in ("not available on a SparseDataset (DESIGN.md section 7)", "TPPCATrainer.train",
                 "HPPCAModel.llk / llks / infer / predict / iterate* and HPPCATrainer.train"):
        assert text in str(err.value), text
    assert sp._handle is None


def test_the_row_compressed_flag(P):
    d, k = 1500, 2
    c, mu = np.random.default_rng(0).standard_normal((d, k)), np.zeros(d)
    with pytest.raises(ValueError, match=r"covers state sizes 1 \.\. 16 and output sizes 1 \.\. 1024 \(got k=2, d=1500\)"):
        P.HPPCAModel(0.5, c, mu)
    with pytest.raises(TypeError):
        P.HPPCAModel(0.5, c, mu, None, True)  # keyword-only
    m = P.HPPCAModel(0.5, c, mu, row_compressed=True)
    assert m.row_compressed and m.output_size == d and not P.HPPCAModel(0.5, c[:9], mu[:9]).row_compressed
    with pytest.raises(ValueError, match="covers state sizes"):  # the state-size limit stays
        P.HPPCAModel(0.5, np.zeros((d, 17)), mu, row_compressed=True)
    # init on a SparseDataset sets it
    sp, _, _ = _case(P)
    a = P.HPPCAModel.init(3, sp, seed=5)
    g = P.PPCAModel.init(3, sp, seed=5)
    assert a.row_compressed and np.array_equal(a.transform, g.transform) and sp._handle is None
    # from_ppca and to_canonical carry it
    assert P.HPPCAModel.from_ppca(P.PPCAModel(0.5, c, mu), row_compressed=True).row_compressed
    assert not P.HPPCAModel.from_ppca(P.PPCAModel(0.5, c[:9], mu[:9])).row_compressed
    can = m.to_canonical()
    assert can.row_compressed and can.output_size == d
    # dump / load / pickle
    back = P.HPPCAModel.load(m.dump())
    assert back.row_compressed and np.array_equal(back.transform, c)
    pk = pickle.loads(pickle.dumps(m))
    assert pk.row_compressed and pk.output_size == d and np.array_equal(pk.transform, c) and pk.isotropic_noise == 0.5
    assert not pickle.loads(pickle.dumps(P.HPPCAModel(0.5, c[:9], mu[:9]))).row_compressed
    # a dump written before the flag existed loads with the flag off; an unflagged model dumps that container
    buf = io.BytesIO()
    np.savez(buf, kind="ppca_rs_amd.HPPCAModel", isotropic_noise=0.5, transform=c[:9], mean=mu[:9])
    assert not P.HPPCAModel.load(buf.getvalue()).row_compressed
    assert "row_compressed" not in np.load(io.BytesIO(P.HPPCAModel(0.5, c[:9], mu[:9]).dump())).files


def test_with_values_and_the_aligned_split(P):
    x, p, w, _, pv = H.case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w, block_rows=7, segment=3)
    pr = sp.with_values(pv)
    ip, ix, vals = pr.csr()
    assert np.array_equal(ip, sp.csr()[0]) and np.array_equal(ix, sp.csr()[1]) and np.array_equal(vals, pv)
    assert np.array_equal(pr.weights(), w) and (pr._block_rows, pr._segment) == (7, 3) and pr._d == 9
    assert pr._handle is None and sp._handle is None and pr._ctx_arg is sp._ctx_arg
    assert np.array_equal(pr._dense()[np.isfinite(x)], p[np.isfinite(x)])
    for bad in (pv[:-1], np.ones((2, 2)), np.where(np.arange(pv.size) == 0, np.nan, pv)):
        with pytest.raises(ValueError):
            sp.with_values(bad)
    # the split is keyed by (seed, row, column): data and precisions split alike, and the parts stay aligned
    (tr, he), (ptr_, phe) = sp.holdout(0.3, 11), pr.holdout(0.3, 11)
    for a, b in ((tr, ptr_), (he, phe)):
        assert np.array_equal(a.csr()[0], b.csr()[0]) and np.array_equal(a.csr()[1], b.csr()[1])
        dense_p = b._dense()
        assert np.array_equal(dense_p[np.isfinite(dense_p)], p[np.isfinite(dense_p)])
    assert tr.nnz + he.nnz == sp.nnz and he.nnz > 0 and tr.holdout_counts == ptr_.holdout_counts
    assert not hasattr(pr, "holdout_counts") and all(d._handle is None for d in (tr, he, ptr_, phe))


def test_the_inputs_of_the_gpu_tests():
    """The seam shape shows the row lengths at which the row pass changes its group width and, under block_rows = 64, the column
    lengths around segment = 8; every precision lies in [2^-10, 2^10] and belongs to a stored entry."""
    x, p, w, _, pv = H.case(*H.SEAM)
    obs = np.isfinite(x)
    lens = obs.sum(axis=1)
    assert list(lens[1:len(H.SEAM_ROWS)]) == H.SEAM_ROWS[1:] and lens[0] == 299 and not obs[0, 5]
    assert {0, 1, 15, 16, 17, 63, 64, 65} <= set(lens)
    per_block = set()
    for r0 in range(0, x.shape[0], 64):
        per_block |= set(obs[r0:r0 + 64].sum(axis=0))
    assert set(H.SEAM_COLUMNS) <= per_block, sorted(per_block)
    for n, d, k in H.SHAPES + [H.SEAM]:
        x, p, w, _, pv = H.case(n, d, k)
        assert np.array_equal(np.isfinite(p), np.isfinite(x)) and pv.min() >= H.LO and pv.max() <= H.HI
        assert np.array_equal(p[np.isfinite(x)], pv)


def test_the_sparse_two_noise_level_case():
    """Thirty restatement steps on the sparse case that justifies the feature: the true precisions end 4.04 degrees from the true
    subspace, unit precisions 26.78 (the figures tests/test_gpu_sparse_h.py takes its midpoint from)."""
    h, g = H.restatement_angles()
    print("true precisions: %.3f degrees from the true subspace; unit precisions: %.3f degrees" % (h, g))
    assert abs(h - H.HETERO_ANGLES[0]) <= 5e-3 and abs(g - H.HETERO_ANGLES[1]) <= 5e-3
    x, p, _, _ = H.hetero_case()
    assert abs(np.isfinite(x).mean() - 0.2) < 0.01 and set(np.round(1 / np.sqrt(p[np.isfinite(p)]), 6)) == {0.3, 3.0}
