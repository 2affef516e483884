"""Held-out scoring of the Student-t and known-precision models and K-fold splits, the part that needs no GPU: the
restated predictives against the chain rule of the families' dense log-densities, the host table of the t predictive, the fold
rule, HeldOutScore.pooled, and the declarations."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import heldout_families_restatement as F
import heldout_restatement as H
import hppca_restatement as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ppca_dataset_holdout_range", "ppca_t_pred_table_host", "ppca_t_heldout_score", "ppca_h_heldout_score")
N, D, K = 40, 12, 3  # the chain-rule case


def _chain_case(seed):
    """x (30 % masked), precisions, the model, and the split (fraction 0.3) with an empty train row (its entries all held) and a row
    with one train entry."""
    x, p, _, (s, c, mu) = HP.case(N, D, K, seed, lo=0.25, hi=4.0)
    p = np.where(HP.observed(x, p), p, 1.0)  # (every finite x has a usable precision here; masks are tested on the GPU side)
    train, held, _ = H.holdout(x, 0.3, seed)
    held[3], train[3] = np.where(np.isfinite(x[3]), x[3], np.nan), np.nan
    o = np.flatnonzero(np.isfinite(x[7]))
    train[7], held[7] = np.nan, np.where(np.isfinite(x[7]), x[7], np.nan)
    train[7, o[0]], held[7, o[0]] = x[7, o[0]], np.nan
    assert np.isfinite(held[3]).sum() > 0 and np.isfinite(train[7]).sum() == 1 and np.isfinite(held[7]).sum() > 0
    return x, p, (s, c, mu), train, held


def _rel(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    return float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max())


@pytest.mark.parametrize("nu", [0.7, 4.0, 50.0])
def test_t_predictive_is_the_chain_rule_of_the_t_density(nu):
    """l of a held entry = ell(train row plus that entry) - ell(train row), the dense m x m t log-density on both sides"""
    _, _, (s, c, mu), train, held = _chain_case(21)
    _, _, l = F.t_entry_scores(train, held, s, c, mu, nu)
    err = _rel(l, F.t_chain(train, held, s, c, mu, nu))
    print("t chain rule nu=%g: %.1e" % (nu, err))
    assert err <= 1e-12


def test_t_variance_rule():
    """v = s nu_m / (nu_m - 2) when nu_m > 2, no variance otherwise: at nu = 0.7 the rows with 0 and 1 train entries have none"""
    _, _, (s, c, mu), train, held = _chain_case(21)
    e, v, l = F.t_entry_scores(train, held, s, c, mu, 0.7)
    m = np.isfinite(train).sum(axis=1)
    fin = np.isfinite(held)
    assert np.all(np.isinf(v[fin & (m[:, None] + 0.7 <= 2.0)])) and np.all(np.isfinite(v[fin & (m[:, None] + 0.7 > 2.0)]))
    assert (m == 0).any() and (m == 1).any() and (m >= 2).any()
    res = H.summarize(e, v, l)
    assert np.isfinite(res["totals"]).all() and res["totals"][4] == fin.sum()


def test_known_precision_predictive_is_the_chain_rule_of_the_density():
    x, p, (s, c, mu), train, held = _chain_case(22)
    _, _, l = F.h_entry_scores(train, p, held, p, s, c, mu)
    err = _rel(l, F.h_chain(train, p, held, p, s, c, mu))
    print("known-precision chain rule: %.1e" % err)
    assert err <= 1e-12
    # every precision 1: the Gaussian restatement
    one = np.ones_like(x)
    a, b = F.h_score(train, one, held, one, s, c, mu), H.score(train, held, s, c, mu)
    assert np.abs(a["per_row"] - b["per_row"]).max() <= 1e-12 * (1.0 + np.abs(b["per_row"]).max())


@pytest.mark.parametrize("nu", [0.7, 4.0, 50.0])
def test_pred_table_against_lgamma(hiplib, nu):
    tbl = np.zeros(D + 1)
    assert hiplib.ppca_t_pred_table_host(D, C.c_double(nu), tbl.ctypes.data_as(C.c_void_p)) == 0
    err = float(np.abs(tbl - F.pred_table(D, nu)).max())
    print("pred table nu=%g: %.1e" % (nu, err))
    assert err <= 1e-13


def test_pred_table_at_a_large_dof(hiplib):
    """ln Gamma(a + 1/2) - ln Gamma(a) - 1/2 ln(2 pi a) = -1/2 ln 2 pi - 1/(8 a) + O(a^-3), a = nu_m / 2: the difference of the two
    lgamma values themselves is off by about 1e-7 here"""
    nu = 1e8
    tbl = np.zeros(D + 1)
    assert hiplib.ppca_t_pred_table_host(D, C.c_double(nu), tbl.ctypes.data_as(C.c_void_p)) == 0
    want = np.array([-0.5 * math.log(2.0 * math.pi) - 1.0 / (4.0 * (nu + m)) for m in range(D + 1)])
    err = float(np.abs(tbl - want).max())
    print("pred table nu=1e8: %.1e (naive lgamma difference: %.1e)" % (err, float(np.abs(F.pred_table(D, nu) - want).max())))
    assert err <= 1e-14
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert hiplib.ppca_t_pred_table_host(D, C.c_double(bad), tbl.ctypes.data_as(C.c_void_p)) != 0


@pytest.mark.parametrize("n_folds", [2, 3, 5, 7])
def test_every_observed_entry_is_in_exactly_one_fold(n_folds):
    n, d, seed = 300, 65, 13
    x = H.split_data(n, d, seed)
    obs = np.isfinite(x)
    times = np.zeros((n, d), dtype=np.int64)
    for train, held, (kept, heldc) in F.kfold(x, n_folds, seed):
        fin = np.isfinite(held)
        times += fin
        assert kept + heldc == obs.sum() and np.array_equal(np.isfinite(train), obs & ~fin)
        assert abs(heldc / obs.sum() - 1.0 / n_folds) <= 5.0 * math.sqrt((1.0 / n_folds) * (1.0 - 1.0 / n_folds) / obs.sum())
    assert np.array_equal(times, obs.astype(np.int64))
    e = F.fold_edges(n_folds)
    assert e[0] == 0.0 and e[-1] == 1.0 and len(e) == n_folds + 1 and all(a < b for a, b in zip(e, e[1:]))


def test_range_from_zero_is_the_fraction_rule():
    x = H.split_data(300, 65, 13)
    for f in H.SPLIT_FRACTIONS:
        a, b = F.holdout_range(x, 0.0, f, 13, row_offset=4), H.holdout(x, f, 13, row_offset=4)
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2]


def test_fold_edges_of_the_package_are_the_restated_ones():
    import ppca_rs_amd as P

    for n_folds in (2, 3, 5, 7, 10):
        assert P.Dataset.fold_edges(n_folds) == F.fold_edges(n_folds)
    with pytest.raises(ValueError):
        P.Dataset.fold_edges(1)


def test_pooled_adds_the_folds():
    import ppca_rs_amd as P

    rng = np.random.default_rng(5)
    parts = [P.HeldOutScore(rng.uniform(0.5, 2.0, (4, 6)), 10 + f, 4 + f, rng.standard_normal(9)) for f in range(3)]
    pooled = P.HeldOutScore.pooled(parts)
    cols = sum(s._cols for s in parts)
    for q, row in zip(("count", "llk", "se", "z2"), cols):
        assert np.array_equal(pooled.columns[q], row)
    assert np.array_equal(pooled.llks, parts[0].llks + parts[1].llks + parts[2].llks)
    assert pooled.n_entries == 33 and pooled.n_rows == 15
    assert pooled.count == float(sum(cols[0].tolist())) and pooled.mean_llk == pooled.llk / pooled.count
    # `+` keeps its shard meaning: rows concatenated
    assert len((parts[0] + parts[1]).llks) == 18
    with pytest.raises(ValueError):
        P.HeldOutScore.pooled([])
    with pytest.raises(ValueError):
        P.HeldOutScore.pooled([parts[0], P.HeldOutScore(np.zeros((4, 6)), 0, 0, np.zeros(8))])


def test_symbols_declared_exported_and_reexported(hiplib):
    import ppca_rs
    import ppca_rs_amd as P

    header = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(hiplib, name) is not None
    for name in ("cross_validate", "heldout_score"):
        assert name in P.__all__ and getattr(ppca_rs, name) is getattr(P, name), name
    for cls, name in ((P.TPPCAModel, "score_heldout"), (P.HPPCAModel, "score_heldout"), (P.TPPCATrainer, "select_state_size"),
                      (P.HPPCATrainer, "select_state_size"), (P.Dataset, "kfold"), (P.Dataset, "holdout_range"), (P.HeldOutScore, "pooled")):
        assert callable(getattr(cls, name)), (cls, name)


def test_the_family_wide_score_routes_by_family():
    """heldout_score(model, ...) wants precisions for an HPPCAModel and refuses them for every other family (checked before any
    dataset is looked at: no GPU is touched); the routing itself is what tests/test_gpu_heldout_families.py runs"""
    import ppca_rs_amd as P

    c, mu = np.ones((4, 2)), np.zeros(4)
    hm, tm, gm = P.HPPCAModel(1.0, c, mu), P.TPPCAModel(1.0, c, mu, 4.0), P.PPCAModel(1.0, c, mu)
    for cls, model in ((P.HPPCAModel, hm), (P.TPPCAModel, tm)):
        assert not hasattr(cls, "heldout_score")  # (tests/test_heldout_host.py pins that name's absence; the method is score_heldout)
    with pytest.raises(ValueError):
        P.heldout_score(hm, None, None)
    with pytest.raises(ValueError):
        P.heldout_score(tm, None, None, precisions=np.ones((1, 4)))
    with pytest.raises(ValueError):
        P.heldout_score(gm, None, None, held_precisions=np.ones((1, 4)))
