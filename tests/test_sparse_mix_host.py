"""CPU-only: the host side of the mixture on a SparseDataset -- the C-ABI table, the refusals Python makes before
the library is touched, and the test inputs themselves (deterministic; finite and unsaturated under the oracle)."""
import re

import numpy as np
import pytest

import sparse_mix_cases as MC

NEW = {"ppca_mix_sparse_llk": 8, "ppca_mix_sparse_component_llks": 5, "ppca_mix_sparse_em_step": 9, "ppca_mix_sparse_predict": 9}


def _header_args(name):
    import os

    import test_abi

    text = open(os.path.join(test_abi.ROOT, "include", "ppca_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
    return len([a for a in args.split(",") if a.strip()])


def test_new_symbols_are_exported_and_declared(hiplib):
    from ppca_rs_amd import _lib

    for name, n_args in NEW.items():
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == _header_args(name) == n_args, name


def _sparse(P):
    return P.SparseDataset([0, 2, 2, 5], [1, 3, 0, 2, 3], np.arange(5.0), 4)


def _mix(P, d=4):
    return P.PPCAMix([P.PPCAModel(1.0, np.ones((d, 2)), np.zeros(d)), P.PPCAModel(0.5, np.ones((d, 1)), np.ones(d))], [0.0, 0.0])


def test_kmeans_start_takes_a_dense_dataset():
    import ppca_rs_amd as P

    sp = _sparse(P)
    with pytest.raises(ValueError, match="k-means takes a dense Dataset"):
        P.PPCAMix.init(2, 2, sp, seed=1, method="kmeans")
    with pytest.raises(ValueError, match="k-means takes a dense Dataset"):
        P.PPCAMix.from_kmeans(2, sp, None)
    with pytest.raises(ValueError, match="k-means takes a dense Dataset"):
        P.PPCAMixTrainer(sp).train(n_models=2, state_size=2, n_iters=1, quiet=True, init="kmeans")
    with pytest.raises(ValueError, match="method must be"):
        P.PPCAMix.init(2, 2, sp, seed=1, method="other")


def test_dense_only_mixture_calls_say_what_the_mixture_offers():
    import ppca_rs_amd as P

    sp, mix = _sparse(P), _mix(P)
    for call in (mix.infer, mix.smooth, mix.extrapolate, mix.sample_posterior, mix.loo_predictive, mix.loo_llks, mix.loo_llk):
        with pytest.raises(TypeError, match="PPCAMix.llk / llks / infer_cluster"):
            call(sp)
    with pytest.raises(TypeError, match="PPCAMix.llk / llks / infer_cluster"):
        mix.heldout_score(sp, sp)
    with pytest.raises(TypeError):
        P.heldout_score(mix, sp, sp)
    with pytest.raises(TypeError, match="SparseDataset"):
        mix.predict(np.zeros((3, 4)), ([0, 0, 0, 0], []))
    with pytest.raises(ValueError):
        mix.predict(sp, ([0, 1, 1], [0]))  # a row short
    with pytest.raises(ValueError):
        mix.predict(sp, ([0, 1, 1, 2], [0, 4]))  # column = d
    with pytest.raises(ValueError):
        mix.iterate(P.SparseDataset([0], [], [], 4))  # empty


def test_init_draws_the_seeds_of_the_dense_start():
    """PPCAMix.init on a SparseDataset needs no device and gives the components it gives on the same data as a (host) pattern: the
    per-component seeds and the zeroed rows of columns without an entry."""
    import ppca_rs_amd as P

    x, w, _, _, _ = MC.mix_case(64, 9, 3, 2)
    sp = P.SparseDataset.from_dense(x, w)
    a, b = P.PPCAMix.init(3, 2, sp, seed=7), P.PPCAMix.init(3, 2, sp, seed=7)
    ss = np.random.SeedSequence(7)
    seeds = [int(s.generate_state(1)[0]) for s in ss.spawn(3)]
    empty = [j for j in range(9) if not np.isfinite(x[:, j]).any()]
    assert 5 in empty
    for c, (ma, mb) in enumerate(zip(a.models, b.models)):
        want = np.random.default_rng(seeds[c]).standard_normal(9 * 2).reshape((2, 9)).T.copy()
        want[empty] = 0.0
        assert np.array_equal(ma.transform, want) and np.array_equal(mb.transform, want)
        assert ma.isotropic_noise == 1.0 and not ma.mean.any()
    assert np.array_equal(a.log_weights, np.log(np.full(3, 1 / 3)))


def test_mix_case_is_deterministic():
    a, b = MC.mix_case(64, 9, 3, 2), MC.mix_case(64, 9, 3, 2)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    x, w, (s, c, mu), lw, labels = a
    assert x.shape == (64, 9) and c.shape == (2, 9, 3) and mu.shape == (2, 9) and s.shape == lw.shape == (2,)
    assert (w > 0).all() and np.exp(lw).sum() == pytest.approx(1.0)
    obs = np.isfinite(x)
    assert obs[0].sum() == 8 and not obs[1].any() and not obs[-1].any() and not obs[:, 5].any()  # row 0: every column but 5
    assert set(labels) == {0, 1}


@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_oracle_is_finite_and_unsaturated(oracle, n, d, k, nm):
    x, w, (s, c, mu), lw, _ = MC.mix_case(n, d, k, nm)
    llks = oracle.mix_llks(x, s, c, mu, lw)
    lp = oracle.mix_infer_cluster(x, s, c, mu, lw)
    s1, c1, m1, lw1 = oracle.mix_iterate(x, s, c, mu, lw, w)
    assert all(np.isfinite(a).all() for a in (llks, lp, s1, c1, m1, lw1))
    soft = float((np.exp(lp).max(axis=1) < 0.99).mean())
    print("%dx%dx%d nm %d: %.0f %% of the rows have a largest posterior below 0.99" % (n, d, k, nm, 100 * soft))
    assert 0.05 <= soft <= 0.6
