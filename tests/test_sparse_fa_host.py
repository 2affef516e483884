"""Factor analysis on row-compressed data, the part that needs no GPU: the cases of tests/sparse_fa_cases.py,
the restatement identities the device path rests on, the new C-ABI symbols, and the argument checks that answer before any device is
touched."""
import ctypes as C

import numpy as np
import pytest

import fa_restatement as R
import sparse_cases as SC
import sparse_fa_cases as F

INVALID, UNSUPPORTED = -1, -3
IDENTITY_SHAPES = [(64, 9, 3), (150, 300, 11), (100, 20, 0)]
STEP_SHAPES = [s for s in F.SHAPES if s[1] <= 2000]


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("n,d,k", [(64, 9, 3), (257, 300, 1), (100, 20, 0)])
def test_fa_case_is_deterministic_and_keeps_the_edges(n, d, k):
    x, w, (noise, c, mu), psi = F.fa_case(n, d, k)
    F.fa_case.cache_clear()
    x2, w2, (noise2, c2, mu2), psi2 = F.fa_case(n, d, k)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in ((x, x2), (w, w2), (noise, noise2), (c, c2), (mu, mu2), (psi, psi2)))
    x0, w0, (s0, c0, mu0) = SC.case(n, d, k)
    obs = np.isfinite(x)
    assert np.array_equal(obs, np.isfinite(x0)) and np.array_equal(w, w0) and c.shape == (d, k)
    assert np.array_equal(x[obs], (x0 * psi)[obs]) and np.array_equal(noise, s0 * psi) and np.array_equal(mu, mu0 * psi)
    assert np.all((psi >= 0.1) & (psi <= 10.0)) and psi.max() / psi.min() > 10.0
    lengths = obs.sum(axis=1)
    assert lengths[0] == d - 1 and lengths[1] == 0 and lengths[-1] == 0  # row 0 has every column but 5; the empty rows
    assert obs[:, 3].sum() == 1 and obs[:, 5].sum() == 0 and np.array_equal(obs[:, 7], lengths > 0)
    assert w[n // 2] == 0.0


def test_the_case_list_covers_what_the_issue_names():
    shapes = {(n, d, k) for n, d, k, t in F.CASES if not t}
    assert shapes == set(F.SHAPES) and (40, 70000, 3) in shapes and (100, 20, 0) in shapes
    sweep = sorted(k for n, d, k, t in F.CASES if (n, d) == (150, 300) and t == F.SWEEP_TILING)
    assert sweep == list(range(17))
    seams = [t for n, d, k, t in F.CASES if (n, d, k) == F.SEAM]
    assert seams == [dict(block_rows=64, segment=8), dict(block_rows=64), dict(segment=8), dict(block_rows=7, segment=3)]


# ------------------------------------------------------------------ the identities the design rests on
@pytest.mark.parametrize("n,d,k", IDENTITY_SHAPES)
def test_llks_equal_the_whitened_ppca_density_minus_the_jacobian(n, d, k):
    """fa_restatement.llks(x, psi, C, mu) = the PPCA log-density of the whitened rows under (1, C / psi, mu / psi) - sum ln psi_j over
    the row's entries, at 1e-10 relative to 1 + |l|; the k x k evaluation of sparse_fa_cases agrees with the m x m one."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    want = R.llks(x, noise, c, mu)
    white = R.llks(x / noise, np.ones(d), c / noise[:, None], mu / noise)  # sigma = 1: the isotropic model's density
    jac = np.where(np.isfinite(x), np.log(noise), 0.0).sum(axis=1)
    err = float((np.abs(white - jac - want) / (1.0 + np.abs(want))).max())
    low = float((np.abs(F.llks_low_rank(x, noise, c, mu) - want) / (1.0 + np.abs(want))).max())
    print("(%d, %d, %d): whitened identity %.2e, k x k form %.2e (bound 1e-10)" % (n, d, k, err, low))
    assert err <= 1e-10 and low <= 1e-10
    assert np.array_equal(F.restatement_llks(x, noise, c, mu), want)


@pytest.mark.parametrize("n,d,k", STEP_SHAPES, ids=["%dx%dx%d" % s for s in STEP_SHAPES])
def test_a_step_in_whitened_units_equals_the_step_in_the_original_ones(n, d, k):
    """One restatement iterate in the original units against the same step formed in whitened units, which is what the device does.
    Measured on the CPU: at most 2.2e-12 / 2.1e-12 / 3.8e-14 (psi / C / mean) on the shapes up to (200, 1500, 16), 7.6e-12 / 8.9e-13 /
    3.6e-15 at (300, 2000, 10).  Pinned at 1e-8: the distance to the project's 1e-5 parity bound is what makes that bound safe for
    these inputs."""
    x, w, (noise, c, mu), _ = F.fa_case(n, d, k)
    zero = F.zero_variance_columns(x, w, k)  # (k = 0, column 3: a new variance of exactly 0, whose rounding is all either side returns)
    white, orig = F.whitened_iterate(x, w, noise, c, mu), R.iterate(x, w, noise, c, mu)
    gaps = F.model_gaps(white, orig, zero)
    print("(%d, %d, %d): psi %.2e, C %.2e, mean %.2e (bound 1e-8); %d zero-variance columns" % ((n, d, k) + gaps + (int(zero.sum()),)))
    assert max(gaps) <= 1e-8
    assert zero.sum() == (1 if k == 0 else 0)
    assert F.zero_variance_outcome(white[0], noise, x, w, mu, zero) and F.zero_variance_outcome(orig[0], noise, x, w, mu, zero)


# ------------------------------------------------------------------ the C-ABI
def test_abi_has_the_new_symbols(hiplib):
    import test_abi
    from ppca_rs_amd import _lib

    for name in ("ppca_scale_columns_sparse", "ppca_fa_sparse_em_step"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES and name in test_abi._declared_symbols()
    test_abi.test_header_symbols_exported(hiplib)
    assert hiplib.ppca_abi_version() == 6


def test_the_routines_refuse_null_arguments(hiplib):
    one = np.ones(3)
    p = one.ctypes.data_as(C.c_void_p)
    assert hiplib.ppca_scale_columns_sparse(None, None, p, None, None, None, p, None) == INVALID and hiplib.ppca_last_error()
    assert hiplib.ppca_fa_sparse_em_step(None, None, 3, 1, p, p, p, None, p, p, p, None) == INVALID


# ------------------------------------------------------------------ the argument checks of the Python layer: no device is touched
def test_argument_checks_come_before_any_device(hiplib):
    import ppca_rs_amd as P

    x, w, (noise, c, mu), _ = F.fa_case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.FAModel(noise, c, mu)
    for bad in (np.nan, np.inf):
        v = np.ones(9)
        v[4] = bad
        for kw in (dict(a=v), dict(a=np.ones(9), b=v), dict(a=np.ones(9), l=v)):
            with pytest.raises(ValueError, match="finite"):
                sp._scale_columns(**kw)
    with pytest.raises(ValueError):
        sp._scale_columns(np.ones(8))  # the wrong length
    with pytest.raises(ValueError, match="no output"):
        sp._scale_columns(np.ones(9), out=False)
    rng = np.random.default_rng(0)
    wide = P.FAModel(np.ones(9), rng.standard_normal((9, 17)), np.zeros(9))
    for call in (wide.llks, wide.llk, wide.infer, wide.iterate, wide.iterate_with_llk, lambda s: wide.predict(s, s),
                 lambda s: wide.heldout_score(s, s)):
        with pytest.raises(P.PPCAError) as err:
            call(sp)
        assert err.value.code == UNSUPPORTED
    other = P.FAModel(np.ones(10), rng.standard_normal((10, 3)), np.zeros(10))
    for call in (other.llks, other.llk, other.infer, other.iterate, lambda s: other.predict(s, s)):
        with pytest.raises(ValueError, match="output size"):
            call(sp)
    with pytest.raises(ValueError, match="empty"):
        model.iterate(P.SparseDataset([0], [], [], 9))
    with pytest.raises(ValueError, match="pca"):
        P.FAModel.init(3, sp, seed=1, method="pca")
    with pytest.raises(ValueError, match="pca"):
        P.FATrainer(sp).train(state_size=3, n_iters=1, seed=1, quiet=True, init="pca")
    for call in (model.smooth, model.extrapolate):
        with pytest.raises(TypeError, match="predict"):
            call(sp)
    with pytest.raises(TypeError):
        model.predict(P.Dataset.__new__(P.Dataset), sp)
    with pytest.raises(ValueError):
        model.predict(sp, (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32)))  # a query of other rows
    train, held = sp.holdout(0.3, 1)
    with pytest.raises(TypeError, match="one of each"):
        model.heldout_score(train, P.Dataset.__new__(P.Dataset))
    with pytest.raises(TypeError, match="one of each"):
        model.heldout_score(P.Dataset.__new__(P.Dataset), held)
    with pytest.raises(ValueError, match="block_rows"):
        model.heldout_score(train, P.SparseDataset.from_dense(x, block_rows=16))
    with pytest.raises(ValueError, match="shape"):
        model.heldout_score(train, P.SparseDataset.from_dense(x[:-1]))
    assert sp._handle is None and train._handle is None and sp._ctx_arg is None  # nothing above reached a device


def test_what_stays_as_it_was(hiplib):
    """The package-level heldout_score keeps refusing every model but a PPCAModel on row-compressed data, an FAModel included, and
    cross_validate with it; the wording of SparseDataset._h keeps what the existing tests match; FAMix is not built."""
    import ppca_rs_amd as P

    x, w, (noise, c, mu), _ = F.fa_case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    train, held = sp.holdout(0.3, 1)
    model = P.FAModel(noise, c, mu)
    with pytest.raises(TypeError, match="FAModel"):
        P.heldout_score(model, train, held)
    with pytest.raises(TypeError, match="FAModel"):
        P.cross_validate(sp, lambda tr: model, folds=3, seed=1)
    with pytest.raises(TypeError) as err:
        sp._h
    for text in ("predict", "PPCAMix.llk / llks / infer_cluster", "FAModel.llk / llks / infer", "FATrainer"):
        assert text in str(err.value)
    mix = P.FAMix(noise, [c, c], [mu, mu], np.log([0.5, 0.5]))
    with pytest.raises(TypeError):
        mix.llks(sp)
    assert sp._handle is None


def test_a_view_is_a_sparse_dataset_whose_values_come_on_demand(hiplib):
    """The host side of a values view, without a device: the properties that do not need the values do not fetch them."""
    import ppca_rs_amd as P

    x, w, _, _ = F.fa_case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    view = P.SparseDataset.__new__(P.SparseDataset)
    view.__dict__.update(sp.__dict__)
    view._vals = None  # (what _scale_columns leaves; the handle is the device's)
    assert view.nnz == sp.nnz and len(view) == 64 and view.output_size() == 9 and view.empty_dimensions() == sp.empty_dimensions()
    assert np.array_equal(view.weights(), w) and view._vals is None
    assert "nnz=%d" % sp.nnz in repr(view) and view._vals is None
