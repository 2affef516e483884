"""Held-out scoring without a GPU: the C-ABI surface; the numpy restatement (tests/heldout_restatement.py) against the CPU oracle
through the identity l(x_j | train row) = llks(train row with x_j added) - llks(train row), for the model, the mixture and the factor
model; the realised share of held entries of every split case the GPU test uses; HeldOutScore's arithmetic."""
import os
import re

import numpy as np
import pytest

import fa_restatement as FA
import heldout_restatement as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_dataset_holdout", "ppca_heldout_score", "ppca_mix_heldout_score")
TOL = 1e-10  # relative to 1 + |l|: two fp64 evaluations of one closed form at d = 7


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def test_symbols_and_surface(hiplib, P):
    from ppca_rs_amd import _lib

    header = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(hiplib, name), name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    import ppca_rs

    assert "HeldOutScore" in P.__all__ and ppca_rs.HeldOutScore is P.HeldOutScore
    assert hasattr(P.Dataset, "holdout")
    for cls in (P.PPCAModel, P.PPCAMix, P.FAModel, P.FAMix):
        assert hasattr(cls, "heldout_score"), cls
    for cls in (P.PPCATrainer, P.FATrainer):
        assert hasattr(cls, "select_state_size"), cls
    for cls in (P.TPPCAModel, P.HPPCAModel):  # out of scope
        assert not hasattr(cls, "heldout_score"), cls


def _one_held_case(d, k, seed, n=14):
    """train / held with exactly one held entry per row (none in the last row), disjoint; row 0 has no train entry, row 1 one."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) * 1.5 + 0.3
    train = x.copy()
    train[rng.random((n, d)) < 0.3] = np.nan
    held = np.full((n, d), np.nan)
    for i in range(n - 1):
        j = int(rng.integers(d))
        held[i, j] = x[i, j]
        train[i, j] = np.nan
    train[0] = np.nan
    keep = int(np.flatnonzero(~np.isfinite(held[1]))[0])
    train[1] = np.nan
    train[1, keep] = x[1, keep]
    c, mu, s = 0.8 * rng.standard_normal((d, k)), 0.4 * rng.standard_normal(d), 0.6
    return train, held, (s, c, mu)


def _with_held(train, held):
    both = train.copy()
    fin = np.isfinite(held)
    assert not (fin & np.isfinite(train)).any()
    both[fin] = held[fin]
    return both


def _close(got, want):
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert err.max() <= TOL, err.max()


@pytest.mark.parametrize("k", [3, 0])
def test_restatement_against_oracle_identity(oracle, k):
    train, held, (s, c, mu) = _one_held_case(7, k, 21 + k)
    want = oracle.llks(_with_held(train, held), s, c, mu) - oracle.llks(train, s, c, mu)
    res = H.score(train, held, s, c, mu)
    _close(res["per_row"], want)
    assert res["per_row"][-1] == 0.0 and res["totals"][4] == len(train) - 1 and res["totals"][5] == len(train) - 1
    # a row with no train entry: the prior predictive (mean_j, sigma^2 + |c_j|^2)
    j = int(np.flatnonzero(np.isfinite(held[0]))[0])
    v = s * s + c[j] @ c[j]
    _close(res["per_row"][0], -0.5 * (H.LN_2PI + np.log(v) + (held[0, j] - mu[j]) ** 2 / v))
    if k > 0:  # fed the oracle's own posteriors: the same numbers
        _close(H.score(train, held, s, c, mu, post=oracle.infer(train, s, c, mu))["per_row"], want)


def _mix_case(seed):
    train, held, _ = _one_held_case(7, 3, seed)
    rng = np.random.default_rng(seed + 100)
    nm = 3
    cs, mus = 0.8 * rng.standard_normal((nm, 7, 3)), rng.standard_normal((nm, 7))
    sig, lw = np.array([0.6, 0.9, 0.4]), np.log(np.array([0.5, 0.3, 0.2]))
    return train, held, sig, cs, mus, lw


def test_mixture_restatement_against_oracle_identity(oracle):
    train, held, sig, cs, mus, lw = _mix_case(31)
    want = oracle.mix_llks(_with_held(train, held), sig, cs, mus, lw) - oracle.mix_llks(train, sig, cs, mus, lw)
    comp = np.stack([oracle.llks(train, s, c, m) for s, c, m in zip(sig, cs, mus)], axis=1)
    res = H.mix_score(train, held, sig, cs, mus, lw, comp)
    _close(res["per_row"], want)
    # a component of log-weight -inf contributes nothing: the mixture of the other two
    lw2 = np.array([np.log(0.6), -np.inf, np.log(0.4)])
    two = H.mix_score(train, held, sig[[0, 2]], cs[[0, 2]], mus[[0, 2]], lw2[[0, 2]], comp[:, [0, 2]])
    three = H.mix_score(train, held, sig, cs, mus, lw2, comp)
    for key in ("per_row", "totals", "col_sums"):
        assert np.array_equal(two[key], three[key]), key
    assert np.isfinite(three["per_row"]).all()


def test_one_component_mixture_equals_the_model(oracle):
    train, held, (s, c, mu) = _one_held_case(7, 3, 41)
    comp = oracle.llks(train, s, c, mu)[:, None]
    one = H.mix_score(train, held, [s], c[None], mu[None], np.zeros(1), comp)
    model = H.score(train, held, s, c, mu)
    for key in ("per_row", "totals", "col_sums"):
        np.testing.assert_allclose(one[key], model[key], rtol=1e-12, atol=0.0)


def test_factor_mapping_against_fa_restatement():
    train, held, (_, c, mu) = _one_held_case(7, 3, 51)
    noise = np.array([0.05, 0.2, 0.7, 1.5, 4.0, 0.01, 9.0])
    want = FA.llks(_with_held(train, held), noise, c, mu) - FA.llks(train, noise, c, mu)
    res = H.fa_score(train, held, noise, c, mu)
    _close(res["per_row"], want)
    # the squared errors are in the units of the data: against the posterior of the un-whitened restatement
    fin = np.isfinite(held)
    se = np.zeros(7)
    for i in np.flatnonzero(fin.any(axis=1)):
        j = int(np.flatnonzero(fin[i])[0])
        z = FA.posterior(train[i], noise, c, mu)[0] if np.isfinite(train[i]).any() else np.zeros(3)
        se[j] += (held[i, j] - mu[j] - c[j] @ z) ** 2
    np.testing.assert_allclose(res["col_sums"][2], se, rtol=1e-9, atol=1e-12)
    assert res["totals"][1] == pytest.approx(res["per_row"].sum(), rel=1e-12)


def test_holdout_rule_basics():
    x = H.split_data(40, 9, 2)
    u = H.holdout_uniforms(40, 9, 77)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(H.holdout_uniforms(10, 9, 77, row_offset=25), u[25:35])  # a shard reproduces its rows
    assert not np.array_equal(H.holdout_uniforms(40, 9, 78), u)
    obs = np.isfinite(x)
    for f in (0.0, 0.3, 1.0):
        train, held, (kept, nh) = H.holdout(x, f, 77)
        assert not (np.isfinite(train) & np.isfinite(held)).any()
        assert np.array_equal(np.isfinite(train) | np.isfinite(held), obs) and kept + nh == obs.sum()
        assert np.array_equal(train[np.isfinite(train)], x[np.isfinite(train)]) and np.array_equal(held[np.isfinite(held)], x[np.isfinite(held)])
    assert H.holdout(x, 0.0, 77)[2][1] == 0 and H.holdout(x, 1.0, 77)[2][0] == 0


@pytest.mark.parametrize("n,d,seed", H.SPLIT_SHAPES)
def test_realised_share_of_the_gpu_cases(n, d, seed):
    """A condition on the seeds the GPU test uses: within 5 standard deviations of a binomial share."""
    x = H.split_data(n, d, seed)
    n_obs = int(np.isfinite(x).sum())
    for f in H.SPLIT_FRACTIONS:
        kept, held = H.holdout(x, f, seed)[2]
        assert kept + held == n_obs
        if n_obs:
            assert abs(held / n_obs - f) <= 5.0 * np.sqrt(f * (1.0 - f) / n_obs), (f, held, n_obs)


def test_heldout_score_adds(P):
    rng = np.random.default_rng(5)
    a = P.HeldOutScore(rng.uniform(1, 2, (4, 6)), 20, 7, rng.standard_normal(7))
    b = P.HeldOutScore(rng.uniform(1, 2, (4, 6)), 31, 9, rng.standard_normal(9))
    s = a + b
    assert s.n_entries == 51 and s.n_rows == 16 and np.array_equal(s.llks, np.concatenate([a.llks, b.llks]))
    for key in ("count", "llk", "se", "z2"):
        assert np.array_equal(s.columns[key], a.columns[key] + b.columns[key])
    assert s.count == pytest.approx(a.count + b.count) and s.llk == pytest.approx(a.llk + b.llk)
    assert s.mean_llk == pytest.approx(s.llk / s.count) and s.mse == pytest.approx(s.columns["se"].sum() / s.count)
    assert s.rmse == pytest.approx(np.sqrt(s.mse)) and s.mean_z2 == pytest.approx(s.columns["z2"].sum() / s.count)
    np.testing.assert_allclose(s.columns["rmse"], np.sqrt(s.columns["se"] / s.columns["count"]))
    with pytest.raises(ValueError):
        a + P.HeldOutScore(np.ones((4, 5)), 1, 1, np.zeros(1))
    empty = P.HeldOutScore(np.zeros((4, 6)), 0, 0, np.zeros(3))
    assert empty.count == 0.0 and np.isnan(empty.mean_llk) and np.isnan(empty.rmse)
