"""Held-out scoring on the GPU: Dataset.holdout against the restated rule bit for bit; heldout_score of PPCAModel,
PPCAMix, FAModel and FAMix against the numpy restatement (tests/heldout_restatement.py); its independence of the grid, the chunking
and the split of the rows; and one end-to-end selection of the state size.

Bounds.  TOL = the project's GPU parity tolerance, 1e-5, against the restatement fed the ORACLE's posteriors (z, Sigma): per row
relative to 1 + |value|, sums relative to the sum of their terms' magnitudes.  TOL_OWN, against the restatement fed the device's own
`infer` output -- the same closed form in fp64 on both sides, so what is left is the order of a few k^2 multiply-adds per entry and
of the sums: 100 x the maximum measured on the MI355X over every shape of SCORE_SHAPES, and no looser than 1e-10.
Every parity check prints its worst error before asserting."""
import ctypes as C

import numpy as np
import pytest

import heldout_restatement as H
import mask_patterns as MP

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_OWN = 1e-10
# N x d x k: the fused posterior pass (d <= 256, k <= 10), the split pipeline's lane solver (k <= 8 of d > 256) and solve4 (k = 16), d > 256,
# a k^2 loop longer than a wave (k = 40), the column sums kept in global memory instead of LDS (1024 x 64), state size 0
SCORE_SHAPES = [(1, 1, 1), (200, 31, 6), (300, 256, 10), (200, 200, 16), (150, 300, 4), (100, 1024, 16), (120, 160, 40), (40, 1024, 64),
                (100, 20, 0)]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _same_bits(got, want):
    """values and NaN positions"""
    fin = np.isfinite(want)
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[fin].view(np.int64), want[fin].view(np.int64))


def _rel_rows(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if len(want) else 0.0


def _rel_sums(got, want, scale):
    return float((np.abs(got - want) / np.maximum(scale, 1e-300)).max())


def _errors(sc, res):
    """HeldOutScore against a restatement result: per row, column sums and totals"""
    cols = sc.columns
    got = np.stack([cols["count"], cols["llk"], cols["se"], cols["z2"]])
    scale = np.where(res["col_abs"] > 0, res["col_abs"], 1.0)
    tot = np.array([sc.count, sc.llk, float(sum(cols["se"].tolist())), float(sum(cols["z2"].tolist()))])  # (index order, as the library's)
    tscale = np.where(res["total_abs"] > 0, res["total_abs"], 1.0)
    return dict(rows=_rel_rows(sc.llks, res["per_row"]), cols=_rel_sums(got, res["col_sums"], scale),
                totals=_rel_sums(tot, res["totals"][:4], tscale))


def _counts_match(sc, res):
    return sc.n_entries == int(res["totals"][4]) and sc.n_rows == int(res["totals"][5])


# ------------------------------------------------------------------ 1. the split
def _check_split(P, x, w, seed):
    from ppca_rs_amd import _lib

    n, d = x.shape
    ds = P.Dataset(x, w)
    ctx = _lib.default_context()
    for f in H.SPLIT_FRACTIONS:
        want_t, want_h, counts = H.holdout(x, f, seed)
        train, held = ds.holdout(f, seed)
        gt, gh = train.numpy(), held.numpy()
        assert _same_bits(gt, want_t) and _same_bits(gh, want_h), (n, d, f)
        assert train.holdout_counts == counts and held.holdout_counts == counts
        assert np.array_equal(train.weights(), w) and np.array_equal(held.weights(), w)
        try:
            ctx.set_grid_limit(3)
            t3, h3 = ds.holdout(f, seed)
            assert _same_bits(t3.numpy(), want_t) and _same_bits(h3.numpy(), want_h) and t3.holdout_counts == counts
        finally:
            ctx.set_grid_limit(0)
        if n >= 3:
            s0, ln = n // 3, n - n // 3 - 1
            ts, hs = ds._slice(s0, ln).holdout(f, seed, row_offset=s0)
            assert _same_bits(ts.numpy(), want_t[s0:s0 + ln]) and _same_bits(hs.numpy(), want_h[s0:s0 + ln])
            assert np.array_equal(ts.weights(), w[s0:s0 + ln])
    if f == 1.0:
        assert not np.isfinite(gt).any()


@pytest.mark.parametrize("n,d,seed", H.SPLIT_SHAPES)
def test_split_matches_the_restated_rule(P, n, d, seed):
    x = H.split_data(n, d, seed)
    if n > 4:
        x[2, 0], x[3, d - 1] = np.inf, -np.inf  # any non-finite value is a masked entry
    _check_split(P, x, np.random.default_rng(seed).uniform(0.25, 2.0, n), seed)


@pytest.mark.parametrize("name", ["full", "rank_edge", "words", "stripe64", "tile_blocks"])
def test_split_under_structured_masks(P, name):
    """full rows, empty rows (rank_edge, tile_blocks) and empty mask words (words, stripe64)"""
    n, d = 257, 256
    x = np.random.default_rng(8).standard_normal((n, d))
    x[~MP.patterns(n, d, 4, 8)[name]] = np.nan
    _check_split(P, x, np.ones(n), 19)


def test_split_rejects_a_bad_fraction(P):
    from ppca_rs_amd import _lib

    ds = P.Dataset(H.split_data(10, 4, 1))
    for f in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ds.holdout(f, 1)
        th, hh = C.c_void_p(), C.c_void_p()
        rc = _lib.lib().ppca_dataset_holdout(ds._ctx.handle, ds._h, f, 1, 0, C.byref(th), C.byref(hh), None)
        assert rc == -1 and not th.value and not hh.value  # PPCA_ERR_INVALID, nothing allocated
    with pytest.raises(ValueError):
        ds.holdout(0.1, 1, row_offset=-1)


def test_split_draws_a_seed_when_none_is_given(P):
    ds = P.Dataset(H.split_data(50, 16, 4))
    a, b = ds.holdout(0.5), ds.holdout(0.5)
    assert sum(a[0].holdout_counts) == sum(b[0].holdout_counts)
    assert not np.array_equal(np.isfinite(a[1].numpy()), np.isfinite(b[1].numpy()))


# ------------------------------------------------------------------ 2. the score against the restatement
_CASES = {}


def _score_case(oracle, n, d, k):
    """x (30 % masked), weights, model, train / held (fraction 0.15; rows without a train entry, rows without a held entry) and the
    oracle's posteriors of the train rows.  Computed once per shape and shared; read-only."""
    key = (n, d, k)
    if key not in _CASES:
        rng = np.random.default_rng(100 + d + k)
        x, _, _ = oracle.synth(n, d, max(k, 1), 0.3, 300 + d + k, sigma_true=0.4)
        train, held, _ = H.holdout(x, 0.15, 50 + d)
        if n >= 20:
            train[3] = np.nan
            train[n - 1] = np.nan
            held[5] = np.nan
            held[n - 2] = np.nan
        c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.7
        w = rng.uniform(0.25, 2.0, n)
        post = oracle.infer(train, s, c, mu) if k > 0 else H.posteriors(train, s, c, mu)
        for a in (x, train, held, c, mu, w) + tuple(post):
            a.setflags(write=False)
        _CASES[key] = (x, w, (s, c, mu), train, held, post)
    return _CASES[key]


@pytest.mark.parametrize("n,d,k", SCORE_SHAPES)
def test_score_matches_the_restatement(P, oracle, n, d, k):
    x, w, (s, c, mu), train, held, post = _score_case(oracle, n, d, k)
    tds, hds, m = P.Dataset(train, w), P.Dataset(held), P.PPCAModel(s, c, mu)
    sc = m.heldout_score(tds, hds)
    res = H.score(train, held, s, c, mu, w=w, post=post)
    errs = _errors(sc, res)
    print("score %dx%dx%d vs oracle posteriors:" % (n, d, k), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert _counts_match(sc, res) and np.all(np.isfinite(sc.llks))
    assert max(errs.values()) <= TOL, errs
    assert np.all(sc.llks[~np.isfinite(held).any(axis=1)] == 0.0)
    if k > 0:  # fed the device's own posteriors
        inf = m.infer(tds)
        own = _errors(sc, H.score(train, held, s, c, mu, w=w, post=(inf._states, inf._covs)))
        print("score %dx%dx%d vs own posteriors:" % (n, d, k), " ".join("%s %.1e" % kv for kv in own.items()), "(bound %g)" % TOL_OWN)
        assert max(own.values()) <= TOL_OWN, own
    again = m.heldout_score(tds, hds)  # two runs: the same bits
    assert np.array_equal(again.llks, sc.llks) and all(np.array_equal(again.columns[q], sc.columns[q]) for q in ("count", "llk", "se", "z2"))


def test_score_edge_datasets(P, oracle):
    n, d, k = 200, 31, 6
    x, w, (s, c, mu), train, held, post = _score_case(oracle, n, d, k)
    m, tds = P.PPCAModel(s, c, mu), P.Dataset(train, w)
    # nothing held: zeros, no NaN
    sc = m.heldout_score(tds, P.Dataset(np.full((n, d), np.nan)))
    assert sc.n_entries == 0 and sc.n_rows == 0 and sc.count == 0.0 and sc.llk == 0.0 and np.all(sc.llks == 0.0)
    assert all(np.all(sc.columns[q] == 0.0) for q in ("count", "llk", "se", "z2"))
    # everything held, train empty: the prior predictive everywhere
    xo = np.where(np.isfinite(x), x, np.nan)
    empty = np.full((n, d), np.nan)
    sc = m.heldout_score(P.Dataset(empty, w), P.Dataset(xo))
    v = s * s + (c * c).sum(axis=1)
    l = np.where(np.isfinite(xo), -0.5 * (H.LN_2PI + np.log(v)[None, :] + (xo - mu[None, :]) ** 2 / v[None, :]), 0.0)
    assert _rel_rows(sc.llks, l.sum(axis=1)) <= TOL_OWN and sc.n_entries == int(np.isfinite(xo).sum())
    # held = train (not disjoint): scored as a new reading of the column
    sc = m.heldout_score(tds, P.Dataset(train))
    errs = _errors(sc, H.score(train, train, s, c, mu, w=w, post=post))
    print("held = train:", errs)
    assert max(errs.values()) <= TOL, errs
    # shapes that differ
    with pytest.raises(ValueError):
        m.heldout_score(tds, P.Dataset(held[:-1]))
    from ppca_rs_amd import _lib

    short = P.Dataset(np.ascontiguousarray(held[:, :-1]))
    tot = np.zeros(6)
    rc = _lib.lib().ppca_heldout_score(tds._ctx.handle, tds._h, short._h, m._device(tds._ctx).h, tot.ctypes.data_as(C.c_void_p), None, None)
    assert rc == -1


@pytest.mark.parametrize("n,d,k", [(300, 256, 10), (300, 300, 4), (300, 200, 16)])
def test_score_grid_chunks_and_slices(P, oracle, monkeypatch, n, d, k):
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(7 + k)
    x, _, _ = oracle.synth(n, d, k, 0.3, 900 + k, sigma_true=0.4)
    train, held, _ = H.holdout(x, 0.15, 33)
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.7
    w = rng.uniform(0.25, 2.0, n)
    tds, hds, m = P.Dataset(train, w), P.Dataset(held), P.PPCAModel(s, c, mu)
    base = m.heldout_score(tds, hds)
    bc = base.columns

    def cols_close(sc):
        for q in ("count", "llk", "se", "z2"):
            scale = np.maximum(np.abs(bc[q]), 1e-300)
            assert (np.abs(sc.columns[q] - bc[q]) / scale).max() <= 1e-12, q

    ctx = _lib.default_context()
    try:
        ctx.set_grid_limit(3)
        sc = m.heldout_score(tds, hds)
        assert np.array_equal(sc.llks, base.llks)
        cols_close(sc)
    finally:
        ctx.set_grid_limit(0)
    for var, val in (("PPCA_HELD_CHUNK", "64"), ("PPCA_GEN_CHUNK", "256")):
        monkeypatch.setenv(var, val)
        sc = m.heldout_score(tds, hds)
        monkeypatch.delenv(var)
        assert np.array_equal(sc.llks, base.llks), var
        cols_close(sc)
        assert sc.n_entries == base.n_entries and sc.n_rows == base.n_rows
    s0, ln = n // 3 + 5, n // 2
    part = m.heldout_score(tds._slice(s0, ln), hds._slice(s0, ln))
    assert np.array_equal(part.llks, base.llks[s0:s0 + ln])


def test_score_agrees_with_extrapolate_and_the_covariance_diagonal(P, oracle):
    n, d, k = 300, 40, 5
    rng = np.random.default_rng(3)
    x, _, _ = oracle.synth(n, d, k, 0.3, 77, sigma_true=0.4)
    c, mu, s = 0.5 * rng.standard_normal((d, k)), 0.2 * rng.standard_normal(d), 0.7
    ds, m = P.Dataset(x), P.PPCAModel(s, c, mu)
    tds, hds = ds.holdout(0.2, 9)
    held = hds.numpy()
    fin = np.isfinite(held)
    e = np.where(fin, held - m.extrapolate(tds).numpy(), np.nan)
    # (the extrapolated covariance diagonal of a masked entry already is sigma^2 + c_j^T Sigma c_j: ppca_model.rs:542-577)
    v = np.where(fin, m.infer(tds).extrapolated_covariances_diagonal(m, tds).numpy(), np.nan)
    res = H.summarize(e, v, -0.5 * (H.LN_2PI + np.log(v) + e * e / v))
    errs = _errors(m.heldout_score(tds, hds), res)
    print("vs extrapolate + covariance diagonal:", errs)
    assert max(errs.values()) <= 1e-12, errs


# ------------------------------------------------------------------ 3. the mixture
def _pad(cs, kmax):
    return np.stack([np.concatenate([c_, np.zeros((c_.shape[0], kmax - c_.shape[1]))], axis=1) for c_ in cs])


def _mix_case(oracle, d, ks, seed):
    rng = np.random.default_rng(seed)
    nm, n = len(ks), 240
    x = np.concatenate([oracle.synth(n // nm, d, 3, 0.3, 500 + c_ + d, mean_scale=2.0)[0] for c_ in range(nm)])
    train, held, _ = H.holdout(x, 0.15, seed)
    train[7] = np.nan
    held[9] = np.nan
    cs = [0.5 * rng.standard_normal((d, k_)) for k_ in ks]
    mus = [rng.standard_normal(d) * 2.0 for _ in ks]
    sig = rng.uniform(0.3, 0.9, nm)
    w = rng.uniform(0.25, 2.0, x.shape[0])
    return train, held, w, sig, cs, mus


def _mix_reference(oracle, train, held, w, sig, cs, mus, lw):
    comp = np.stack([oracle.llks(train, s, c, mu) for s, c, mu in zip(sig, cs, mus)], axis=1)
    posts = [oracle.infer(train, s, c, mu) for s, c, mu in zip(sig, cs, mus)]
    return H.mix_score(train, held, sig, cs, mus, lw, comp, w=w, posts=posts)


@pytest.mark.parametrize("d,ks", [(20, (3, 5, 2)), (300, (4, 6))])
def test_mixture_matches_the_restatement(P, oracle, d, ks):
    train, held, w, sig, cs, mus = _mix_case(oracle, d, ks, 19 + d)
    lw = np.log(np.random.default_rng(d).dirichlet(np.ones(len(ks))))
    mix = P.PPCAMix([P.PPCAModel(s, c, mu) for s, c, mu in zip(sig, cs, mus)], lw)
    tds, hds = P.Dataset(train, w), P.Dataset(held)
    sc = mix.heldout_score(tds, hds)
    res = _mix_reference(oracle, train, held, w, sig, cs, mus, lw)
    errs = _errors(sc, res)
    print("mixture d=%d ks=%s:" % (d, ks), " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert _counts_match(sc, res) and max(errs.values()) <= TOL, errs
    again = mix.heldout_score(tds, hds)
    assert np.array_equal(again.llks, sc.llks) and np.array_equal(again.columns["z2"], sc.columns["z2"])


def test_mixture_with_a_component_of_weight_zero(P, oracle):
    train, held, w, sig, cs, mus = _mix_case(oracle, 20, (3, 5, 2), 61)
    lw = np.array([np.log(0.7), -np.inf, np.log(0.3)])
    tds, hds = P.Dataset(train, w), P.Dataset(held)
    models = [P.PPCAModel(s, c, mu) for s, c, mu in zip(sig, cs, mus)]
    sc = P.PPCAMix(models, lw).heldout_score(tds, hds)
    assert np.all(np.isfinite(sc.llks)) and np.isfinite(sc.llk) and np.isfinite(sc.mean_z2)
    errs = _errors(sc, _mix_reference(oracle, train, held, w, sig[[0, 2]], [cs[0], cs[2]], [mus[0], mus[2]], lw[[0, 2]]))
    print("weight-zero component:", errs)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("n,d,k", [(200, 31, 6), (150, 300, 4)])
def test_one_component_mixture_equals_the_model(P, oracle, n, d, k):
    x, w, (s, c, mu), train, held, post = _score_case(oracle, n, d, k)
    tds, hds, m = P.Dataset(train, w), P.Dataset(held), P.PPCAModel(s, c, mu)
    a, b = m.heldout_score(tds, hds), P.PPCAMix([m], np.zeros(1)).heldout_score(tds, hds)
    same = np.array_equal(a.llks, b.llks) and all(np.array_equal(a.columns[q], b.columns[q]) for q in ("count", "llk", "se", "z2"))
    print("one component %dx%dx%d: bit-identical to the model: %s" % (n, d, k, same))  # (the kernel is arranged for it: DESIGN.md 4.17)
    np.testing.assert_allclose(b.llks, a.llks, rtol=1e-12, atol=0.0)
    for q in ("count", "llk", "se", "z2"):
        np.testing.assert_allclose(b.columns[q], a.columns[q], rtol=1e-12, atol=0.0, err_msg=q)
    assert (a.n_entries, a.n_rows) == (b.n_entries, b.n_rows)


# ------------------------------------------------------------------ 4. the factor models
def test_factor_models_match_the_restatement(P, oracle):
    n, d, k = 200, 24, 3
    rng = np.random.default_rng(12)
    noise = 10.0 ** rng.uniform(-2.0, 1.0, d)  # three decades
    c, mu = rng.standard_normal((d, k)) * noise[:, None], rng.standard_normal(d)
    x = rng.standard_normal((n, k)) @ c.T + mu + noise * rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.3] = np.nan
    train, held, _ = H.holdout(x, 0.2, 5)
    train[4] = np.nan
    w = rng.uniform(0.25, 2.0, n)
    tds, hds = P.Dataset(train, w), P.Dataset(held)
    sc = P.FAModel(noise, c, mu).heldout_score(tds, hds)
    res = H.fa_score(train, held, noise, c, mu, w=w)
    errs = _errors(sc, res)
    print("FAModel:", " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert _counts_match(sc, res) and max(errs.values()) <= TOL, errs
    # FAMix: two components sharing the noise
    c2, mu2 = rng.standard_normal((d, k)) * noise[:, None], mu + 3.0 * noise * rng.standard_normal(d)
    lw = np.log(np.array([0.6, 0.4]))
    sc = P.FAMix(noise, np.stack([c, c2]), np.stack([mu, mu2]), lw).heldout_score(tds, hds)
    tw, hw = train / noise, held / noise
    cw, mw = [c / noise[:, None], c2 / noise[:, None]], [mu / noise, mu2 / noise]
    comp = np.stack([oracle.llks(tw, 1.0, a, b) for a, b in zip(cw, mw)], axis=1)
    res = H.unwhiten(H.mix_score(tw, hw, [1.0, 1.0], cw, mw, lw, comp, w=w), held, noise)
    errs = _errors(sc, res)
    print("FAMix:", " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)
    assert _counts_match(sc, res) and max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ 5. end to end
def test_select_state_size_finds_the_true_one(P, oracle):
    """Data of a true k = 3 model (N = 600, d = 12, 30 % masked, noise 0.5): the held-out mean log-density peaks at k = 3 while the
    in-sample log-likelihood of the same six models only grows with k.  The CPU reference alone (the oracle's EM from the same
    starts, scored by the restatement) shows this ordering for this data and seed: held-out -1.9328, -1.6157, -1.0224, -1.0315,
    -1.0355, -1.0374; in-sample -8283.3, -7610.8, -6106.4, -6097.2, -6092.0, -6090.3."""
    x, _, _ = oracle.synth(600, 12, 3, 0.3, 13, sigma_true=0.5)
    ds = P.Dataset(x)
    out = P.PPCATrainer(ds).select_state_size(range(1, 7), fraction=0.15, seed=7, n_iters=30)
    assert [k for k, _, _ in out] == [1, 2, 3, 4, 5, 6]
    held = [sc.mean_llk for _, sc, _ in out]
    train, _ = ds.holdout(0.15, 7)
    insample = [m.llk(train) for _, _, m in out]
    print("held-out mean llk", held, "in-sample llk", insample)
    assert int(np.argmax(held)) == 2
    assert all(b >= a for a, b in zip(insample, insample[1:]))
    fa = P.FATrainer(ds).select_state_size([2, 3], fraction=0.15, seed=7, n_iters=5)
    assert [k for k, _, _ in fa] == [2, 3] and all(np.isfinite(sc.mean_llk) for _, sc, _ in fa)
