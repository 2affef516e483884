"""CPU-only: the host side of PPCAMix.recommend -- the C-ABI symbol, the argument checks (each raises before
the library or a device is touched), the restated combination of tests/mix_topn_cases.py against exact rational arithmetic, and the
inputs of the GPU tests (unsaturated responsibilities under the oracle)."""
from fractions import Fraction

import numpy as np
import pytest

import mix_topn_cases as XC
import sparse_cases as SC
import topn_cases as TC

UNSUPPORTED = -3
NAME, N_ARGS = "ppca_mix_topn_sparse", 12


def test_abi_has_the_mixture_topn_symbol(hiplib):
    import test_abi
    import test_sparse_mix_host as H
    from ppca_rs_amd import _lib

    assert NAME in test_abi._declared_symbols() and hasattr(hiplib, NAME) and NAME in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NAME][1]) == H._header_args(NAME) == N_ARGS
    test_abi.test_header_symbols_exported(hiplib)


def _sparse_and_mix(k=3):
    import ppca_rs_amd as P

    x, w, (s, c, mu) = SC.case(64, 9, 3)
    rng = np.random.default_rng(0)
    models = [P.PPCAModel(s, c, mu), P.PPCAModel(0.9, rng.standard_normal((9, k)), mu + 1.0)]
    return P, P.SparseDataset.from_dense(x, w), P.PPCAMix(models, [0.0, -1.0])


def _untouched(sp, mix):
    return sp._handle is None and sp._ctx_arg is None and all(m._dev is None for m in mix.models)


BAD = {
    "n = 0": dict(n=0),
    "n = 65": dict(n=65),
    "n negative": dict(n=-1),
    "unsorted candidates": dict(n=3, candidates=[0, 4, 2]),
    "repeated candidates": dict(n=3, candidates=[0, 2, 2]),
    "candidate = d": dict(n=3, candidates=[0, 2, 9]),
    "negative candidate": dict(n=3, candidates=[-1, 2]),
    "candidates not integer": dict(n=3, candidates=[0.5, 2.0]),
    "candidates 2-D": dict(n=3, candidates=[[0, 1]]),
    "kappa NaN": dict(n=3, kappa=float("nan")),
    "kappa inf": dict(n=3, kappa=float("inf")),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_rejected_inputs_raise_before_any_device_work(what):
    P, sp, mix = _sparse_and_mix()
    with pytest.raises(ValueError):
        mix.recommend(sp, **BAD[what])
    assert _untouched(sp, mix)


def test_a_dense_dataset_names_the_constructor():
    P, sp, mix = _sparse_and_mix()
    with pytest.raises(TypeError, match="SparseDataset.from_dense"):
        mix.recommend(P.Dataset.__new__(P.Dataset), 3)
    with pytest.raises(TypeError, match="SparseDataset.from_dense"):
        mix.recommend(np.zeros((4, 9)), 3)


def test_state_size_17_in_any_component_is_refused_like_every_sparse_pass():
    P, sp, mix = _sparse_and_mix(k=17)
    with pytest.raises(P.PPCAError) as err:
        mix.recommend(sp, 3)
    assert err.value.code == UNSUPPORTED and _untouched(sp, mix)
    other = P.PPCAMix([P.PPCAModel(1.0, np.ones((10, 2)), np.zeros(10))] * 2, [0.0, 0.0])
    with pytest.raises(ValueError):  # another number of columns
        other.recommend(sp, 3)
    assert _untouched(sp, other)


def test_no_rows_give_empty_results_without_a_device():
    import ppca_rs_amd as P

    mix = P.PPCAMix([P.PPCAModel(1.0, np.ones((3, 2)), np.zeros(3)), P.PPCAModel(1.0, np.ones((3, 0)), np.zeros(3))], [0.0, 0.0])
    sp = P.SparseDataset([0], [], [], 3)
    cols, scores = mix.recommend(sp, 4, candidates=[])
    assert cols.shape == scores.shape == (0, 4) and cols.dtype == np.int32 and scores.dtype == np.float64
    assert _untouched(sp, mix)


def test_the_sparse_dataset_names_recommend_among_the_mixture_calls():
    import ppca_rs_amd as P

    with pytest.raises(TypeError, match=r"PPCAMix.llk / llks / infer_cluster .* recommend and PPCAMixTrainer"):
        P.SparseDataset([0], [], [], 3)._h


# ------------------------------------------------------------------ the restated combination
def _exact_fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _exact_moments(m, v, r):
    """mix_moments of one (row, column) in exact rationals, rounded once where the library rounds once."""
    mean, var = float(Fraction(r[0]) * Fraction(m[0])), float(Fraction(r[0]) * Fraction(v[0]))
    for c in range(1, len(m)):
        mean, var = _exact_fma(r[c], m[c], mean), _exact_fma(r[c], v[c], var)
    s = 0.0
    for c in range(len(m)):
        dv = float(Fraction(m[c]) - Fraction(mean))
        s = _exact_fma(r[c], float(Fraction(dv) * Fraction(dv)), s)
    return mean, float(Fraction(var) + Fraction(s))


@pytest.mark.parametrize("nm", [1, 2, 3, 5])
def test_mix_score_rounds_where_the_library_rounds(nm):
    rng = np.random.default_rng(10 + nm)
    n, d = 40, 25  # 1000 (row, column) pairs per nm
    means = 3.0 * rng.standard_normal((nm, n, d)) + 2.0 * rng.standard_normal((nm, 1, 1))
    vars_ = 0.3 + rng.random((nm, n, d)) * 10.0 ** rng.integers(-2, 2, (nm, n, d))
    post = rng.dirichlet(np.full(nm, 0.7), n)
    post[0] = 0.0
    post[0, nm - 1] = 1.0  # a saturated row: the other weights are exactly 0
    mean, var = XC.mix_moments(means, vars_, post)
    want = np.array([[_exact_moments(means[:, i, j].tolist(), vars_[:, i, j].tolist(), post[i].tolist()) for j in range(d)] for i in range(n)])
    assert np.array_equal(mean, want[:, :, 0]) and np.array_equal(var, want[:, :, 1])
    if nm > 1:  # (two roundings per step do differ somewhere on this set)
        plain = sum(post.T[c][:, None] * means[c] for c in range(nm))
        assert not np.array_equal(plain, mean)
    for kappa in XC.KAPPAS:
        got = XC.mix_score(means, vars_, post, kappa)
        if kappa == 0:
            assert np.array_equal(got, mean)
            continue
        root = np.sqrt(var)
        exact = np.array([_exact_fma(kappa, a, b) for a, b in zip(root.ravel().tolist(), mean.ravel().tolist())]).reshape(n, d)
        assert np.array_equal(got, exact)


def test_mix_score_of_one_component_is_the_models_score():
    rng = np.random.default_rng(3)
    mean, var = rng.standard_normal((1, 30, 40)), 0.2 + rng.random((1, 30, 40))
    for kappa in XC.KAPPAS:
        got = XC.mix_score(mean, var, np.ones((30, 1)), kappa)
        assert np.array_equal(got.view(np.int64), TC.score(mean[0], var[0], kappa).view(np.int64))


def test_mix_score_of_equal_components_is_the_components_score_to_rounding():
    rng = np.random.default_rng(4)
    mean, var = rng.standard_normal((30, 40)), 0.2 + rng.random((30, 40))
    post = rng.dirichlet(np.full(4, 1.0), 30)
    for kappa in XC.KAPPAS:
        got = XC.mix_score(np.stack([mean] * 4), np.stack([var] * 4), post, kappa)
        want = TC.score(mean, var, kappa)
        assert np.abs(got - want).max() <= 16 * np.finfo(float).eps * (1.0 + np.abs(want).max() + abs(kappa) * np.sqrt(var.max()))


# ------------------------------------------------------------------ the inputs of the GPU tests
def test_seam_rows_have_the_lengths_of_the_single_model_seams():
    for d in XC.SEAM_DS:
        x = XC.seam_case(d)[0]
        assert x.shape == (XC.SEAM_N, d) and tuple(np.isfinite(x).sum(axis=1)[:6]) == XC.seam_lengths(d)


def test_tie_case_ties_in_every_component():
    x, w, (s, c, mu), lw, same = XC.tie_case()
    assert c.shape == (2, 200, 4) and not np.isfinite(x[:, same]).any()
    for e in range(2):
        assert all(np.array_equal(c[e][same[0]], c[e][j]) and mu[e][same[0]] == mu[e][j] for j in same)
    assert not np.array_equal(c[0][10], c[1][10]) and mu[0][10] != mu[1][10]


_UNSATURATED = XC.unsaturated_cases()


@pytest.mark.parametrize("label", sorted(_UNSATURATED))
def test_oracle_responsibilities_are_not_saturated(oracle, label):
    x, _, (s, c, mu), lw, _ = _UNSATURATED[label]()
    lp = oracle.mix_infer_cluster(x, s, c, mu, lw)
    assert np.isfinite(lp).all()
    soft = np.exp(lp).max(axis=1) < 0.99
    print("%s: %.3f of the rows (%d) have a largest posterior below 0.99" % (label, soft.mean(), soft.sum()))
    assert soft.sum() >= 2
