"""SparseDataset on the GPU: the row pass and the column pass over row-compressed data against the oracle on the
densified data and against the library's own dense path; predict; the seams of the tiling (row-length bins, runs of long columns, row
blocks); what the passes promise exactly (per-row outputs that depend on the row alone, a statistics buffer that does not depend on the
grid); errors; and a shape the dense layout cannot hold.

Tolerance: the project's GPU parity bound, 1e-5, with the measures of tests/test_gpu_hppca.py: per-row values relative to 1 + |value|,
sums relative to the sum of their terms' magnitudes, sigma relative, C against max |C|, mean_j against max(|mean_j|, sigma).  Each check
prints its worst error before asserting.  The mean prior is checked at d <= 300, the other two priors at every shape: the mean prior
takes a d x d covariance, and the library's host branch for it (ppca_capi.hip, smooth_mean_host: one LU of the d x d matrix per column
of its inverse, O(d^4)) needs 12 minutes on the host at d = 1500 (measured) -- no test of seconds can cross it."""
import functools

import numpy as np
import pytest

import sparse_cases as SC
import state_size_cases as S

pytestmark = pytest.mark.gpu

TOL = 1e-5
INVALID, UNSUPPORTED, EMPTY = -1, -3, -4
SHAPES = [(1, 1, 1), (64, 9, 3), (257, 300, 1), (300, 2000, 10), (150, 300, 11), (200, 1500, 16), (40, 70000, 3)]
IDS = ["%dx%dx%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(n, d, k, forced=None):
    x, w, model = SC.case(n, d, k, forced=forced)
    _freeze(x, w, *model[1:])
    return x, w, model


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _sum_err(got, want, scale):
    return float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max()) if want.size else 0.0


def _layout(d, k):
    kp = k * (k + 1) // 2
    edges = np.cumsum([0, d * k, d * kp, d * k, d, d, 8])
    return dict(zip(["cross", "S", "U", "sumx", "totals", "scalars"], zip(edges[:-1], edges[1:])))


def _stat_scale(x, w, model, z, cov, llks):
    """The packed statistics with every term replaced by its magnitude (the scale of a sum's rounding), row by row over the observed
    entries."""
    s, c, mu = model
    n, d = x.shape
    k = c.shape[1]
    kp = k * (k + 1) // 2
    il = np.tril_indices(k)
    cross, S, U = np.zeros((d, k)), np.zeros((d, kp)), np.zeros((d, k))
    sumx, totals, sc = np.zeros(d), np.zeros(d), np.zeros(8)
    for i in range(n):
        o = np.flatnonzero(np.isfinite(x[i]))
        xt = x[i, o] - mu[o]
        cross[o] += np.abs(w[i] * xt[:, None] * z[i][None, :])
        S[o] += np.abs(w[i] * (cov[i] + np.outer(z[i], z[i]))[il])[None, :]
        U[o] += np.abs(w[i] * z[i])[None, :]
        sumx[o] += np.abs(w[i] * xt)
        totals[o] += abs(w[i])
        if o.size:
            co = c[o]
            sc[0] += abs(w[i]) * abs(np.trace(cov[i] @ co.T @ co))
            sc[1] += abs(w[i]) * float(xt @ xt)  # the identity's largest term
            sc[4] += 1
        sc[2] += abs(w[i] * llks[i])
        sc[3] += abs(w[i])
    return np.concatenate([cross.ravel(), S.ravel(), U.ravel(), sumx, totals, sc])


@functools.lru_cache(maxsize=None)
def _want(oracle, n, d, k, forced=None):
    x, w, model = _case(n, d, k, forced)
    s, c, mu = model
    llks = oracle.llks(x, s, c, mu)
    z, cov = oracle.infer(x, s, c, mu)
    stats = oracle.stats(x, s, c, mu, w)
    out = dict(llks=llks, llk=oracle.llk(x, s, c, mu, w), z=z, cov=cov, stats=stats, scale=_stat_scale(x, w, model, z, cov, llks))
    _freeze(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


def _stats_errors(got, want, scale, d, k):
    errs = {}
    for name, (a, b) in _layout(d, k).items():
        hi = b - 3 if name == "scalars" else b  # (the last three scalars are unused)
        errs[name] = _sum_err(got[a:hi], want[a:hi], scale[a:hi])
    return errs


def _model_errors(new, want):
    s1, c1, m1 = want
    cmax = np.abs(c1).max() if c1.size else 1.0
    return dict(sigma=abs(new.isotropic_noise / s1 - 1), C=float(np.abs(new.transform - c1).max() / (cmax or 1.0)) if c1.size else 0.0,
                mean=float((np.abs(new.mean - m1) / np.maximum(np.abs(m1), s1)).max()))


def _stats_raw(P, model, sp):
    import ctypes as C

    from ppca_rs_amd._lib import lib, check, ptr

    k = max(model.state_size, 1)
    out = np.empty(int(lib().ppca_stats_len(model.output_size, k)))
    check(lib().ppca_sparse_stats_raw(sp._ctx.handle, sp._sh, model._device(sp._ctx).h, ptr(out)))
    return out


def _dense_stats_raw(model, ds):
    from ppca_rs_amd._lib import lib, check, ptr

    out = np.empty(int(lib().ppca_stats_len(model.output_size, max(model.state_size, 1))))
    check(lib().ppca_stats_raw(ds._ctx.handle, ds._h, model._device(ds._ctx).h, ptr(out)))
    return out


def _show(label, errs):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n,d,k", SHAPES, ids=IDS)
def test_against_oracle(P, oracle, n, d, k):
    _check_against_oracle(P, oracle, n, d, k)


def _check_against_oracle(P, oracle, n, d, k, **tiling):
    x, w, (s, c, mu) = _case(n, d, k)
    e = _want(oracle, n, d, k)
    sp = P.SparseDataset.from_dense(x, w, **tiling)
    model = P.PPCAModel(s, c, mu)
    inf = model.infer(sp)
    errs = dict(llks=_rel(model.llks(sp), e["llks"]), llk=abs(model.llk(sp) - e["llk"]) / max(e["scale"][-6], 1.0),
                z=_rel(inf.states(), e["z"]), Sigma=_rel(np.array(inf.covariances()), e["cov"]))
    _show("rows %dx%dx%d %s" % (n, d, k, tiling or ""), errs)
    assert max(errs.values()) <= TOL, errs
    empty = ~np.isfinite(x).any(axis=1)
    assert np.all(model.llks(sp)[empty] == 0) and not inf.states()[empty].any()
    assert all(np.array_equal(cv, np.eye(k)) for cv in np.array(inf.covariances())[empty])

    got = _stats_raw(P, model, sp)
    serr = _stats_errors(got, e["stats"], e["scale"], d, k)
    _show("   stats", serr)
    assert max(serr.values()) <= TOL, serr
    a, b = _layout(d, k)["totals"]
    assert np.array_equal(_stats_raw(P, model, P.SparseDataset.from_dense(x, **tiling))[a:b], np.isfinite(x).sum(axis=0))  # un-weighted: exact

    new, llk = model.iterate_with_llk(sp)
    merr = _model_errors(new, oracle.iterate(x, s, c, mu, w))
    _show("   iterate", merr)
    assert max(merr.values()) <= TOL, merr
    assert abs(llk - e["llk"]) / max(e["scale"][-6], 1.0) <= TOL
    again = model.iterate(sp)
    assert again.isotropic_noise == new.isotropic_noise and np.array_equal(again.transform, new.transform)

    rng = np.random.default_rng(5)
    prior, oprior = P.Prior().with_isotropic_noise_prior(2.0, 3.0).with_transformation_precision(0.7), oracle.Prior(
        isotropic_noise_alpha=2.0, isotropic_noise_beta=3.0, transformation_precision=0.7)
    if d <= 300:
        a_ = rng.standard_normal((d, d)) / np.sqrt(d)
        pm, pc = rng.standard_normal(d), a_ @ a_.T + np.eye(d)
        prior = prior.with_mean_prior(pm, pc)
        oprior.mean, oprior.mean_covariance = pm, pc
    perr = _model_errors(model.iterate_with_prior(sp, prior), oracle.iterate(x, s, c, mu, w, oprior))
    _show("   iterate_with_prior", perr)
    assert max(perr.values()) <= TOL, perr


@pytest.mark.parametrize("n,d,k", SHAPES, ids=IDS)
def test_predict(P, oracle, n, d, k):
    _check_predict(P, oracle, n, d, k)


def _check_predict(P, oracle, n, d, k):
    x, w, (s, c, mu) = _case(n, d, k)
    e = _want(oracle, n, d, k)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(s, c, mu)
    smooth = oracle.reconstruct(x, s, c, mu, "smooth")
    obs = np.isfinite(x)
    rng = np.random.default_rng(11)
    free = ~obs & (rng.random(x.shape) < min(1.0, 40.0 / d))
    free[::3] = False  # empty query rows
    for name, q in (("observed", obs), ("disjoint", free)):
        rows, cols = np.nonzero(q)
        indptr = np.concatenate([[0], np.cumsum(q.sum(axis=1))])
        mean, var = model.predict(sp, (indptr, cols))
        want_var = np.einsum("ea,eab,eb->e", c[cols], e["cov"][rows], c[cols]) + s * s
        errs = dict(mean=_rel(mean, smooth[rows, cols]), var=_rel(var, want_var))
        _show("predict %s %dx%dx%d (%d entries)" % (name, n, d, k, rows.size), errs)
        assert max(errs.values()) <= TOL, errs
    m2, v2 = model.predict(sp, sp)  # a SparseDataset as the query: its pattern
    rows, cols = np.nonzero(obs)
    assert _rel(m2, smooth[rows, cols]) <= TOL and m2.shape == v2.shape == (sp.nnz,)


# ------------------------------------------------------------------ against the library's dense path
@pytest.mark.parametrize("n,d,k", SHAPES[:-1] + [(64, 9, 0), (257, 300, 0)], ids=IDS[:-1] + ["64x9x0", "257x300x0"])
def test_against_dense_path(P, oracle, n, d, k):
    _check_against_dense_path(P, oracle, n, d, k)


def _check_against_dense_path(P, oracle, n, d, k, **tiling):
    x, w, (s, c, mu) = _case(n, d, k)
    sp = P.SparseDataset.from_dense(x, w, **tiling)
    ds = sp.to_dense()
    assert np.array_equal(np.isfinite(ds.numpy()), np.isfinite(x)) and np.array_equal(ds.weights(), w)
    model = P.PPCAModel(s, c, mu)
    a, b = model.infer(sp), model.infer(ds)
    dl = model.llks(ds)
    errs = dict(llks=_rel(model.llks(sp), dl), llk=abs(model.llk(sp) - model.llk(ds)) / max(float(np.abs(w * dl).sum()), 1.0))
    if k > 0:
        errs.update(z=_rel(a.states(), b.states()), Sigma=_rel(np.array(a.covariances()), np.array(b.covariances())))
        z, cov = b.states(), np.array(b.covariances())
    else:
        z, cov = np.zeros((n, 1)), np.ones((n, 1, 1))
    kk = max(k, 1)
    scale = _stat_scale(x, w, (s, c if k else np.zeros((d, 1)), mu), z, cov, dl)
    errs.update(_stats_errors(_stats_raw(P, model, sp), _dense_stats_raw(model, ds), scale, d, kk))
    new_s, new_d = model.iterate(sp), model.iterate(ds)
    errs.update({"it_" + key: v for key, v in _model_errors(new_s, (new_d.isotropic_noise, new_d.transform, new_d.mean)).items()})
    _show("dense path %dx%dx%d %s" % (n, d, k, tiling or ""), errs)
    assert max(errs.values()) <= TOL, errs
    assert new_s.state_size == k


# ------------------------------------------------------------------ every state size
SWEEP_N, SWEEP_D = S.SPARSE
SWEEP_TILING = dict(block_rows=64, segment=8)  # three row blocks; columns of up to 148 entries cut into runs of 8


@pytest.mark.parametrize("k", range(17))
def test_state_size_sweep(P, oracle, k):
    """Every instantiation of the row and the column kernel (k = 0 is the model without a transform) on rows in all three length bins
    (tests/test_state_sizes_host.py), at the default tiling and at one with three row blocks and every long column cut into runs."""
    check = _check_against_oracle if k else _check_against_dense_path  # (the oracle has no k = 0)
    check(P, oracle, SWEEP_N, SWEEP_D, k)
    check(P, oracle, SWEEP_N, SWEEP_D, k, **SWEEP_TILING)


@pytest.mark.parametrize("k", range(17))
def test_predict_state_size_sweep(P, oracle, k):
    if k:
        return _check_predict(P, oracle, SWEEP_N, SWEEP_D, k)
    x, w, (s, c, mu) = _case(SWEEP_N, SWEEP_D, 0)  # no transform: the column's mean and sigma^2 at every position
    rows, cols = np.nonzero(~np.isfinite(x) & (np.random.default_rng(11).random(x.shape) < 40.0 / SWEEP_D))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=SWEEP_N))])
    mean, var = P.PPCAModel(s, c, mu).predict(P.SparseDataset.from_dense(x, w), (indptr, cols))
    errs = dict(mean=_rel(mean, mu[cols]), var=_rel(var, np.full(cols.size, s * s)))
    _show("predict disjoint %dx%dx0 (%d entries)" % (SWEEP_N, SWEEP_D, rows.size), errs)
    assert rows.size > 1000 and max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ seams
SEAM = (300, 300, 4)
SEAM_ROWS = (15, 16, 17, 63, 64, 65, 300)


def _seam_case():
    """Rows 0-5 of exactly 15, 16, 17, 63, 64, 65 entries and row 6 with every column but one; rows 64-127 (a whole block at
    block_rows = 64) empty; columns 20-25 with 0, 1, 7, 8, 9 and 17 entries (runs of segment = 8: none, one short, one full, one full and
    a remainder, two full and a remainder)."""
    n, d, k = SEAM
    rng = np.random.default_rng(3)
    obs = SC.pattern(n, d, k, rng, forced=(0,) * 7)
    obs[64:128] = False
    obs[:, 20:26] = False
    for i, m in enumerate(SEAM_ROWS[:6]):
        obs[i, 30 + rng.choice(d - 30, size=m, replace=False)] = True
    obs[6] = True
    obs[6, 20] = False
    others = np.r_[7:64, 128:n - 1]
    for j, cnt in ((21, 1), (22, 7), (23, 8), (24, 9), (25, 17)):
        obs[rng.choice(others, size=cnt - 1, replace=False), j] = True
    model = SC.true_model(d, k, rng)
    x = SC.sample(obs, model, rng)
    w = 0.5 + rng.random(n)
    w[n // 2] = 0.0
    _freeze(x, w)
    return x, w, SC.scoring_model(model, rng)


def test_seams(P, oracle):
    n, d, k = SEAM
    x, w, (s, c, mu) = _seam_case()
    lengths = np.isfinite(x).sum(axis=1)
    assert (lengths[64:128] == 0).all() and tuple(np.isfinite(x).sum(axis=0)[20:26]) == (0, 1, 7, 8, 9, 17)
    assert tuple(lengths[:7]) == SEAM_ROWS[:6] + (d - 1,)
    model = P.PPCAModel(s, c, mu)
    z, cov = oracle.infer(x, s, c, mu)
    llks = oracle.llks(x, s, c, mu)
    want, scale = oracle.stats(x, s, c, mu, w), _stat_scale(x, w, (s, c, mu), z, cov, llks)
    for br, seg in ((64, 8), (64, None), (None, 8), (7, 3)):
        sp = P.SparseDataset.from_dense(x, w, block_rows=br, segment=seg)
        errs = _stats_errors(_stats_raw(P, model, sp), want, scale, d, k)
        errs["llks"] = _rel(model.llks(sp), llks)
        _show("seams block_rows=%s segment=%s" % (br, seg), errs)
        assert max(errs.values()) <= TOL, errs


def test_row_lengths_at_the_bin_edges(P, oracle):
    """Rows of exactly 15, 16, 17, 63, 64, 65 and d entries (no edge columns moving them)."""
    n, d, k = 7, 300, 4
    rng = np.random.default_rng(9)
    model = SC.scoring_model(SC.true_model(d, k, rng), rng)
    obs = np.zeros((n, d), dtype=bool)
    for i, m in enumerate(SEAM_ROWS):
        obs[i, rng.choice(d, size=m, replace=False)] = True
    x = SC.sample(obs, model, rng)
    assert tuple(np.isfinite(x).sum(axis=1)) == SEAM_ROWS
    sp = P.SparseDataset.from_dense(x)
    m = P.PPCAModel(*model)
    inf = m.infer(sp)
    z, cov = oracle.infer(x, *model)
    errs = dict(llks=_rel(m.llks(sp), oracle.llks(x, *model)), z=_rel(inf.states(), z), Sigma=_rel(np.array(inf.covariances()), cov))
    _show("bin edges", errs)
    assert max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ determinism
def test_determinism(P):
    n, d, k = SEAM
    x, w, (s, c, mu) = _seam_case()
    model = P.PPCAModel(s, c, mu)
    sp = P.SparseDataset.from_dense(x, w, block_rows=64, segment=8)
    whole = P.SparseDataset.from_dense(x, w, block_rows=n, segment=8)
    ctx = sp._ctx
    ref = (model.llks(sp), model.infer(sp).states(), np.array(model.infer(sp).covariances()))
    ref_stats = {id(sp): _stats_raw(P, model, sp), id(whole): _stats_raw(P, model, whole)}
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            for ds in (sp, whole):
                inf = model.infer(ds)
                got = (model.llks(ds), inf.states(), np.array(inf.covariances()))
                assert all(np.array_equal(g, r) for g, r in zip(got, ref)), (limit, "per-row outputs")
                assert np.array_equal(_stats_raw(P, model, ds), ref_stats[id(ds)]), (limit, "statistics")
    finally:
        ctx.set_grid_limit(0)
    inf = model.infer(whole)
    assert np.array_equal(model.llks(whole), ref[0]) and np.array_equal(inf.states(), ref[1])
    # a row's outputs do not depend on its position or its neighbours: the second half alone, other weights
    half = P.SparseDataset.from_dense(x[150:], np.ones(150))
    assert np.array_equal(model.llks(half), ref[0][150:]) and np.array_equal(model.infer(half).states(), ref[1][150:])
    # additive over row shards
    first = P.SparseDataset.from_dense(x[:150], w[:150])
    second = P.SparseDataset.from_dense(x[150:], w[150:])
    total = _stats_raw(P, model, first) + _stats_raw(P, model, second)
    z, cov = ref[1], ref[2]
    scale = _stat_scale(x, w, (s, c, mu), z, cov, ref[0])
    errs = _stats_errors(total, ref_stats[id(whole)], scale, d, k)
    _show("two halves", errs)
    assert max(errs.values()) <= TOL, errs


# ------------------------------------------------------------------ errors
def test_errors(P):
    x, w, (s, c, mu) = _case(64, 9, 3)
    sp = P.SparseDataset.from_dense(x, w)
    rng = np.random.default_rng(0)
    with pytest.raises(P.PPCAError) as err:
        P.PPCAModel(1.0, rng.standard_normal((9, 17)), np.zeros(9)).llk(sp)
    assert err.value.code == UNSUPPORTED
    with pytest.raises(P.PPCAError) as err:
        P.PPCAModel(1.0, rng.standard_normal((10, 3)), np.zeros(10)).llks(sp)
    assert err.value.code == INVALID
    empty = P.SparseDataset([0], [], [], 9)
    model = P.PPCAModel(s, c, mu)
    with pytest.raises(P.PPCAError) as err:
        model.llk(empty)
    assert err.value.code == EMPTY
    with pytest.raises(ValueError):
        model.iterate(empty)
    with pytest.raises(TypeError):
        model.loo_llk(sp)
    assert np.array_equal(sp.with_weights(np.ones(64)).weights(), np.ones(64))
    assert model.llk(sp.with_weights(2 * w)) == pytest.approx(2 * model.llk(sp), rel=1e-12)


# ------------------------------------------------------------------ capacity
def test_capacity(P, capsys):
    """N = 100 000 x d = 500 000 with 20 entries per row: 400 GB as a dense array.  Three trainer iterations do not lower the
    log-likelihood, and predict on entries kept aside beats each column's training mean."""
    n, d, k, per = 100_000, 500_000, 4, 20
    rng = np.random.default_rng(2024)
    c_true, mu_true = rng.standard_normal((d, k)), rng.standard_normal(d)
    hot = 2000  # most entries fall on a few columns, so that they are learnable from 100 000 rows
    cols = np.where(rng.random((n, per)) < 0.9, rng.integers(0, hot, (n, per)), rng.integers(0, d, (n, per)))
    cols.sort(axis=1)
    keep = np.concatenate([np.ones((n, 1), dtype=bool), np.diff(cols, axis=1) > 0], axis=1)  # no duplicate within a row
    z = rng.standard_normal((n, k))
    vals = np.einsum("nk,npk->np", z, c_true[cols]) + mu_true[cols] + 0.5 * rng.standard_normal((n, per))
    held = keep & (rng.random((n, per)) < 0.1)
    train = keep & ~held

    def csr(mask):
        return np.concatenate([[0], np.cumsum(mask.sum(axis=1))]), cols[mask].astype(np.int32), vals[mask]

    sp = P.SparseDataset(*csr(train), d)
    q_indptr, q_cols, q_vals = csr(held)
    assert sp.nnz > 1_500_000 and q_vals.size > 150_000
    start = P.PPCAModel.init(k, sp, seed=1)
    llks = []
    model = start
    for _ in range(3):
        model, llk = model.iterate_with_llk(sp)
        llks.append(llk)
    llks.append(model.llk(sp))
    print("capacity: llk", llks, "index build %.2f s" % sp.index_build_seconds())
    assert all(b >= a for a, b in zip(llks, llks[1:])), llks
    trained = P.PPCATrainer(sp).train(start=start, state_size=k, n_iters=3, quiet=True)
    assert trained.llk(sp) == pytest.approx(llks[-1], rel=1e-7)
    model = P.PPCATrainer(sp).train(start=model, state_size=k, n_iters=12, quiet=True)  # (three iterations from a random start are no fit yet)

    mean, var = model.predict(sp, (q_indptr, q_cols))
    t_indptr, t_cols, t_vals = sp.csr()
    cnt = np.bincount(t_cols, minlength=d)
    col_mean = np.bincount(t_cols, weights=t_vals, minlength=d) / np.maximum(cnt, 1)
    seen = cnt[q_cols] > 0
    rmse = float(np.sqrt(np.mean((mean[seen] - q_vals[seen]) ** 2)))
    base = float(np.sqrt(np.mean((col_mean[q_cols][seen] - q_vals[seen]) ** 2)))
    print("capacity: held-out rmse %.4f against the column means' %.4f over %d entries" % (rmse, base, int(seen.sum())))
    assert rmse < base and np.all(var > 0)
