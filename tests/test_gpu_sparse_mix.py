"""PPCAMix on a SparseDataset on the GPU: the mixture's row pass, EM step and predict over row-compressed data
against the oracle on the densified data and against the library's own dense mixture; what the passes promise exactly (ell_c of a row
is PPCAModel.llks' bit for bit; per-row outputs that depend on the row alone; a step that does not depend on the grid); the seams of
the tiling; components of different state sizes; errors.

Tolerance: the project's GPU parity bound, 1e-5, with the measures of tests/test_gpu_sparse.py: per-row values relative to 1 + |value|,
sigma relative, C against max |C|, mean_j against max(|mean_j|, sigma), log-weights relative to 1 + |value|; predict's mean relative to
max(|mean|, sqrt(var)) and its variance relative.  Each check prints its worst error before asserting.  The mean prior is checked at
d <= 300 only, for the reason in that file's docstring.

The comparison with the dense mixture's step leaves out the (component, column) pairs the dense step does not resolve (_unresolved:
1 to 11 pairs a shape) and holds the sparse step to the oracle there; measured without that, the two steps differ by 0.56 of max |C|
and 0.08 in the mean at (64, 9, 3, nm 2), column 3 of component 0, where the sparse step agrees with the oracle to 8e-15."""
import functools

import numpy as np
import pytest

import sparse_mix_cases as MC

pytestmark = pytest.mark.gpu

TOL = 1e-5
# The (component, column) pairs that _unresolved takes out of the comparison with the dense step, per shape, as counted when the test
# was written (a property of the inputs and of the dense mixture's posteriors, not of the sparse step): the exclusion may not grow.
UNRESOLVED = dict(zip(MC.SHAPES, (1, 2, 2, 1, 1, 11)))
INVALID, UNSUPPORTED, EMPTY = -1, -3, -4


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(n, d, k, nm):
    x, w, (s, c, mu), lw, _ = MC.mix_case(n, d, k, nm)
    _freeze(x, w, s, c, mu, lw)
    return x, w, (s, c, mu), lw


def _mix(P, model, lw, sizes=None):
    s, c, mu = model
    sizes = [c.shape[2]] * len(s) if sizes is None else sizes
    return P.PPCAMix([P.PPCAModel(s[i], np.ascontiguousarray(c[i][:, :sizes[i]]), mu[i]) for i in range(len(s))], lw)


def _rel(got, want):
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max()) if want.size else 0.0


def _show(label, errs):
    print(label, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %g)" % TOL)


def _mix_errors(new, want, skip=None):
    """want: (sigmas, cs, means, log_weights) of the reference step; the worst component under each measure.  skip (nm, d) bool: the
    (component, column) pairs left out of C and mean (_unresolved)."""
    s1, c1, m1, lw1 = want
    errs = dict(sigma=0.0, C=0.0, mean=0.0, logw=_rel(new.log_weights, np.asarray(lw1)))
    for i, m in enumerate(new.models):
        k = m.state_size
        keep = np.ones(m.mean.shape[0], dtype=bool) if skip is None else ~skip[i]
        ci = np.asarray(c1[i])[:, :k]
        cmax = np.abs(ci).max() if ci.size else 1.0
        errs["sigma"] = max(errs["sigma"], abs(m.isotropic_noise / s1[i] - 1))
        if ci.size:
            errs["C"] = max(errs["C"], float(np.abs(m.transform - ci)[keep].max(initial=0.0) / (cmax or 1.0)))
        errs["mean"] = max(errs["mean"], float((np.abs(m.mean - m1[i]) / np.maximum(np.abs(m1[i]), s1[i]))[keep].max(initial=0.0)))
    return errs


def _unresolved(mix, ds, x, w):
    """The (component, column) pairs (nm, d) that the DENSE mixture step does not resolve: columns with entries whose total weight
    under the component, sum_i w_i r_ic over the rows that observe the column, is below 2^-53 of the component's largest row weight.
    The dense component pass adds every row's terms into statistics that it forms relative to the pass's largest terms (the int8
    slices behind their fp64 guard, and below 2^-200 the rows are dropped altogether: ppca_capi.hip, mix_component_enqueue); what lies
    below the fp64 resolution of those is rounding there, while the column's own solve is scale-free -- the weight cancels -- and the
    sparse step, which adds a column's terms among themselves only, resolves it (measured at 64 x 9, k = 3: column 3, observed in row
    0 alone at e^-99 of component 0's largest weight; the dense step is off by 1.05 in C there, the sparse step agrees with the oracle
    to 8e-15).  These pairs are left out of the comparison of the two steps and checked against the oracle instead (_against_oracle)."""
    with np.errstate(divide="ignore"):
        u = np.log(w)[:, None] + mix.infer_cluster(ds)
    rel = np.exp(u - u.max(axis=0))
    obs = (np.isfinite(x) & (w > 0)[:, None]).astype(float)
    return (rel.T @ obs < 2.0 ** -53) & (obs.sum(axis=0) > 0)[None, :]


def _against_oracle(oracle, new, skip, x, w, model, lw):
    """The sparse step at the pairs of `skip` against the oracle; rows of weight 0 contribute nothing, and the oracle takes none: it
    runs without them."""
    if not skip.any():
        return {}
    s, c, mu = model
    live = w > 0
    want = oracle.mix_iterate(x[live], s, c, mu, lw, w[live])
    return {"skipped_" + key: v for key, v in _mix_errors(new, want, ~skip).items() if key in ("C", "mean")}


def _of_mix(mix):
    return ([m.isotropic_noise for m in mix.models], [m.transform for m in mix.models], [m.mean for m in mix.models], mix.log_weights)


def _same_mix(a, b):
    return (np.array_equal(a.log_weights, b.log_weights) and
            all(p.isotropic_noise == q.isotropic_noise and np.array_equal(p.transform, q.transform) and np.array_equal(p.mean, q.mean)
                for p, q in zip(a.models, b.models)))


def _component_llks(mix, sp):
    from ppca_rs_amd._lib import lib, check, ptr

    devs, arr = mix._handles(sp._ctx)
    out = np.empty((len(devs), len(sp)))
    check(lib().ppca_mix_sparse_component_llks(sp._ctx.handle, sp._sh, arr, len(devs), ptr(out)))
    return out


def _patterns(x, seed=11):
    """The observed pattern and a disjoint one with empty query rows, as (rows, cols, indptr)."""
    obs = np.isfinite(x)
    rng = np.random.default_rng(seed)
    free = ~obs & (rng.random(x.shape) < min(1.0, 40.0 / x.shape[1]))
    free[::3] = False
    out = {}
    for name, q in (("observed", obs), ("disjoint", free)):
        rows, cols = np.nonzero(q)
        out[name] = (rows, cols.astype(np.int32), np.concatenate([[0], np.cumsum(q.sum(axis=1))]).astype(np.int64))
    return out


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_against_oracle(P, oracle, n, d, k, nm):
    x, w, (s, c, mu), lw = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, (s, c, mu), lw)
    want_llks = oracle.mix_llks(x, s, c, mu, lw)
    want_lp = oracle.mix_infer_cluster(x, s, c, mu, lw)
    llks, lp = mix.llks(sp), mix.infer_cluster(sp)
    errs = dict(llks=_rel(llks, want_llks), llk=abs(mix.llk(sp) - float(w @ want_llks)) / max(float(np.abs(w * want_llks).sum()), 1.0),
                logpost=_rel(lp, want_lp))
    _show("mix rows %dx%dx%d nm %d" % (n, d, k, nm), errs)
    assert max(errs.values()) <= TOL, errs
    empty = ~np.isfinite(x).any(axis=1)
    assert empty.any() and np.allclose(lp[empty], mix.log_weights, rtol=0, atol=1e-14) and np.allclose(llks[empty], 0.0, atol=1e-14)

    new, llk = mix.iterate_with_llk(sp)
    ierr = _mix_errors(new, oracle.mix_iterate(x, s, c, mu, lw, w))
    _show("   iterate", ierr)
    assert max(ierr.values()) <= TOL, ierr
    assert abs(llk - float(w @ want_llks)) / max(float(np.abs(w * want_llks).sum()), 1.0) <= TOL
    assert _same_mix(mix.iterate(sp), new)

    rng = np.random.default_rng(5)
    prior, oprior = P.Prior().with_isotropic_noise_prior(2.0, 3.0).with_transformation_precision(0.7), oracle.Prior(
        isotropic_noise_alpha=2.0, isotropic_noise_beta=3.0, transformation_precision=0.7)
    if d <= 300:
        a_ = rng.standard_normal((d, d)) / np.sqrt(d)
        pm, pc = rng.standard_normal(d), a_ @ a_.T + np.eye(d)
        prior = prior.with_mean_prior(pm, pc)
        oprior.mean, oprior.mean_covariance = pm, pc
    perr = _mix_errors(mix.iterate_with_prior(sp, prior), oracle.mix_iterate(x, s, c, mu, lw, w, oprior))
    _show("   iterate_with_prior", perr)
    assert max(perr.values()) <= TOL, perr


# ------------------------------------------------------------------ against the library's dense mixture, one weight 0
@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_against_dense_mixture_with_a_zero_weight(P, oracle, n, d, k, nm):
    x, w, model, lw = _case(n, d, k, nm)
    w = w.copy()
    w[n // 2] = 0.0
    sp = P.SparseDataset.from_dense(x, w)
    ds = sp.to_dense()
    mix = _mix(P, model, lw)
    dl = mix.llks(ds)
    errs = dict(llks=_rel(mix.llks(sp), dl), logpost=_rel(mix.infer_cluster(sp), mix.infer_cluster(ds)))
    (new_s, llk_s), (new_d, llk_d) = mix.iterate_with_llk(sp), mix.iterate_with_llk(ds)
    skip = _unresolved(mix, ds, x, w)
    errs.update(_mix_errors(new_s, _of_mix(new_d), skip))
    errs.update(_against_oracle(oracle, new_s, skip, x, w, model, lw))
    errs["llk"] = abs(llk_s - llk_d) / max(float(np.abs(w * dl).sum()), 1.0)
    _show("dense mixture %dx%dx%d nm %d (%d of %d (component, column) pairs against the oracle instead)" % (n, d, k, nm, skip.sum(), skip.size),
          errs)
    assert max(errs.values()) <= TOL, errs
    assert skip.sum() <= UNRESOLVED[n, d, k, nm], "more pairs than recorded are left to the oracle"


# ------------------------------------------------------------------ bit-identity
@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_component_llks_are_the_single_models_bit_for_bit(P, n, d, k, nm):
    x, w, model, lw = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw)
    got = _component_llks(mix, sp)
    for c, m in enumerate(mix.models):
        assert np.array_equal(got[c], m.llks(sp)), "component %d" % c


@pytest.mark.parametrize("k", range(17))
def test_component_llks_bit_for_bit_at_every_state_size(P, k):
    """The mixture's row kernel repeats the single model's statements instead of sharing a function with it, so every instantiation
    is held to the single model's bits: rows of all three length bins (row 0 is full), both forms of the kernel."""
    x, w, model, lw = _case(150, 300, k, 2)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, model, lw)
    got = _component_llks(mix, sp)
    lengths = np.isfinite(x).sum(axis=1)
    assert (lengths <= 16).any() and ((lengths > 16) & (lengths <= 64)).any() and (lengths > 64).any()
    for c, m in enumerate(mix.models):
        want = m.llks(sp)
        bad = np.flatnonzero(got[c] != want)
        print("k %d component %d: %d of %d rows differ, lengths %s" % (k, c, bad.size, len(want), sorted(set(lengths[bad]))[:8]))
        assert bad.size == 0, "component %d" % c


@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_determinism(P, n, d, k, nm):
    x, w, model, lw = _case(n, d, k, nm)
    mix = _mix(P, model, lw)
    sp = P.SparseDataset.from_dense(x, w, block_rows=64, segment=8)
    whole = P.SparseDataset.from_dense(x, w, block_rows=n, segment=8)
    pats = _patterns(x)
    query = [(p[2], p[1]) for p in pats.values()]

    def outputs(ds, qs):
        return [mix.llks(ds), mix.infer_cluster(ds)] + [a for q in qs for a in mix.predict(ds, q)]

    ref = outputs(sp, query)
    steps = {id(sp): mix.iterate(sp), id(whole): mix.iterate(whole)}
    ctx = sp._ctx
    try:
        for limit in (1, 3):
            ctx.set_grid_limit(limit)
            for ds in (sp, whole):
                assert all(np.array_equal(g, r) for g, r in zip(outputs(ds, query), ref)), (limit, "per-row outputs")
                assert _same_mix(mix.iterate(ds), steps[id(ds)]), (limit, "iterate")
    finally:
        ctx.set_grid_limit(0)
    assert all(np.array_equal(g, r) for g, r in zip(outputs(whole, query), ref))
    # a row's outputs do not depend on its position or its neighbours: the second half as its own dataset, other weights
    h = n // 2
    half = P.SparseDataset.from_dense(x[h:], np.ones(n - h))
    hq = [(p[2][h:] - p[2][h], p[1][p[2][h]:]) for p in pats.values()]
    cut = [ref[0][h:], ref[1][h:]] + [a[p[2][h]:] for p, (m_, v_) in zip(pats.values(), zip(ref[2::2], ref[3::2])) for a in (m_, v_)]
    assert all(np.array_equal(g, r) for g, r in zip(outputs(half, hq), cut))


# ------------------------------------------------------------------ seams
SEAM = (300, 300, 4, 3)
SEAM_ROWS = (15, 16, 17, 63, 64, 65, 300)


def _seam_edit(obs, rng):
    """Rows 0-5 of exactly 15, 16, 17, 63, 64, 65 entries, row 6 with all d; rows 64-127 (a whole block at block_rows = 64) empty."""
    d = obs.shape[1]
    obs[:7] = False
    for i, m in enumerate(SEAM_ROWS[:6]):
        obs[i, 30 + rng.choice(d - 30, size=m, replace=False)] = True
    obs[6] = True
    obs[64:128] = False


def test_seams(P, oracle):
    n, d, k, nm = SEAM
    x, w, (s, c, mu), lw, _ = MC.mix_case(n, d, k, nm, forced=SEAM_ROWS, edit=_seam_edit)
    lengths = np.isfinite(x).sum(axis=1)
    assert tuple(lengths[:7]) == SEAM_ROWS and (lengths[64:128] == 0).all()
    mix = _mix(P, (s, c, mu), lw)
    want_llks, want_lp = oracle.mix_llks(x, s, c, mu, lw), oracle.mix_infer_cluster(x, s, c, mu, lw)
    want_step = oracle.mix_iterate(x, s, c, mu, lw, w)
    for br, seg in ((64, 8), (64, None), (None, 8), (7, 3)):
        sp = P.SparseDataset.from_dense(x, w, block_rows=br, segment=seg)
        errs = dict(llks=_rel(mix.llks(sp), want_llks), logpost=_rel(mix.infer_cluster(sp), want_lp))
        errs.update(_mix_errors(mix.iterate(sp), want_step))
        _show("seams block_rows=%s segment=%s" % (br, seg), errs)
        assert max(errs.values()) <= TOL, errs
        got = _component_llks(mix, sp)
        assert all(np.array_equal(got[e], m.llks(sp)) for e, m in enumerate(mix.models))


# ------------------------------------------------------------------ components of different state sizes; one component
@pytest.mark.parametrize("n,d,sizes", [(64, 9, (3, 1, 0)), (150, 300, (10, 11))], ids=["64x9-k3,1,0", "150x300-k10,11"])
def test_mixed_state_sizes(P, oracle, n, d, sizes):
    nm, kmax = len(sizes), max(sizes)
    x, w, (s, c, mu), lw = _case(n, d, kmax, nm)
    cz = c.copy()
    for i, k in enumerate(sizes):
        cz[i][:, k:] = 0.0  # the oracle takes one state size: the missing columns as zeros
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, (s, c, mu), lw, sizes)
    assert mix.state_sizes == list(sizes)
    errs = dict(llks=_rel(mix.llks(sp), oracle.mix_llks(x, s, cz, mu, lw)),
                logpost=_rel(mix.infer_cluster(sp), oracle.mix_infer_cluster(x, s, cz, mu, lw)))
    _show("mixed sizes %s" % (sizes,), errs)
    assert max(errs.values()) <= TOL, errs
    got = _component_llks(mix, sp)
    assert all(np.array_equal(got[e], m.llks(sp)) for e, m in enumerate(mix.models))
    ds = sp.to_dense()
    new_s, new_d, skip = mix.iterate(sp), mix.iterate(ds), _unresolved(mix, ds, x, w)
    ierr = _mix_errors(new_s, _of_mix(new_d), skip)
    ierr.update(_against_oracle(oracle, new_s, skip, x, w, (s, cz, mu), lw))
    _show("   iterate against the dense mixture (%d of %d pairs against the oracle instead)" % (skip.sum(), skip.size), ierr)
    assert max(ierr.values()) <= TOL and skip.sum() <= 2, ierr  # (2 of 27 and 1 of 600 pairs as recorded)
    assert new_s.state_sizes == list(sizes)


@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES[:2] + MC.SHAPES[3:4], ids=MC.IDS[:2] + MC.IDS[3:4])
def test_one_component_is_the_single_model(P, n, d, k, nm):
    x, w, (s, c, mu), _ = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    model = P.PPCAModel(s[0], c[0], mu[0])
    mix = P.PPCAMix([model], [0.3])
    assert np.array_equal(mix.llks(sp), model.llks(sp)) and not mix.infer_cluster(sp).any()
    new, want = mix.iterate(sp), model.iterate(sp)
    errs = _mix_errors(new, ([want.isotropic_noise], [want.transform], [want.mean], [0.0]))
    _show("one component %dx%dx%d" % (n, d, k), errs)
    assert max(errs.values()) <= TOL and new.log_weights[0] == 0.0, errs
    for rows, cols, indptr in _patterns(x).values():
        (m1, v1), (m2, v2) = mix.predict(sp, (indptr, cols)), model.predict(sp, (indptr, cols))
        assert np.array_equal(m1, m2) and np.array_equal(v1, v2)


# ------------------------------------------------------------------ predict
@pytest.mark.parametrize("n,d,k,nm", MC.SHAPES, ids=MC.IDS)
def test_predict(P, oracle, n, d, k, nm):
    x, w, (s, c, mu), lw = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    mix = _mix(P, (s, c, mu), lw)
    r = np.exp(oracle.mix_infer_cluster(x, s, c, mu, lw))
    post = [oracle.infer(x, s[e], c[e], mu[e]) for e in range(nm)]
    for name, (rows, cols, indptr) in _patterns(x).items():
        m = np.stack([mu[e][cols] + np.einsum("ea,ea->e", c[e][cols], post[e][0][rows]) for e in range(nm)])
        v = np.stack([np.einsum("ea,eab,eb->e", c[e][cols], post[e][1][rows], c[e][cols]) + s[e] ** 2 for e in range(nm)])
        re = r[rows].T
        want_mean = (re * m).sum(axis=0)
        want_var = (re * v).sum(axis=0) + (re * (m - want_mean) ** 2).sum(axis=0)
        mean, var = mix.predict(sp, (indptr, cols))
        errs = dict(mean=float((np.abs(mean - want_mean) / np.maximum(np.abs(want_mean), np.sqrt(want_var))).max()),
                    var=float((np.abs(var - want_var) / want_var).max()))
        _show("mix predict %s %dx%dx%d nm %d (%d entries)" % (name, n, d, k, nm, rows.size), errs)
        assert rows.size > 0 and max(errs.values()) <= TOL, errs
    rows, cols, indptr = _patterns(x)["observed"]
    (m2, v2), (m3, v3) = mix.predict(sp, sp), mix.predict(sp, (indptr, cols))  # a SparseDataset as the query: its pattern
    assert np.array_equal(m2, m3) and np.array_equal(v2, v3) and m2.shape == v2.shape == (sp.nnz,)


# ------------------------------------------------------------------ training
def test_llk_is_monotone_and_the_trainer_iterates(P):
    n, d, k, nm = 600, 40, 2, 3
    x, w, _, _ = _case(n, d, k, nm)
    sp = P.SparseDataset.from_dense(x, w)
    start = P.PPCAMix.init(3, 2, sp, seed=1)
    dense_start = P.PPCAMix.init(3, 2, sp.to_dense(), seed=1)
    assert _same_mix(start, dense_start)  # the same per-component seeds as on a Dataset
    mix, llks, third = start, [], None
    for it in range(6):
        mix, llk = mix.iterate_with_llk(sp)
        llks.append(llk)
        if it == 2:
            third = mix
    print("mixture llk over six iterations:", llks)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(llks, llks[1:])), llks
    trained = P.PPCAMixTrainer(sp).train(n_models=3, state_size=2, n_iters=3, quiet=True, seed=1)
    assert _same_mix(trained, third.to_canonical())  # (every trainer returns the canonical form)


# ------------------------------------------------------------------ errors
def test_errors(P):
    x, w, (s, c, mu), lw = _case(64, 9, 3, 2)
    sp = P.SparseDataset.from_dense(x, w)
    good = _mix(P, (s, c, mu), lw)
    rng = np.random.default_rng(0)
    wide = P.PPCAMix([good.models[0], P.PPCAModel(1.0, rng.standard_normal((9, 17)), np.zeros(9))], lw)
    other = P.PPCAMix([P.PPCAModel(1.0, rng.standard_normal((10, 3)), np.zeros(10))] * 2, lw)
    empty = P.SparseDataset([0], [], [], 9)
    query = (np.zeros(65, dtype=np.int64), np.zeros(0, dtype=np.int32))
    for mix, ds, code in ((wide, sp, UNSUPPORTED), (other, sp, INVALID), (good, empty, EMPTY)):
        calls = [lambda: mix.llk(ds), lambda: mix.llks(ds), lambda: mix.infer_cluster(ds)]
        if ds is sp:
            calls += [lambda: mix.iterate(ds), lambda: mix.predict(ds, query)]
        for call in calls:
            with pytest.raises(P.PPCAError) as err:
                call()
            assert err.value.code == code, (code, err.value)
    with pytest.raises(ValueError):
        good.iterate(empty)

    import ctypes as C

    from ppca_rs_amd._lib import lib, ptr

    ctx = sp._ctx
    devs, arr = good._handles(ctx)
    out, lw_out = np.empty((2, 64)), np.empty(2)
    assert lib().ppca_mix_sparse_llk(ctx.handle, sp._sh, arr, ptr(lw), 0, None, None, None) == INVALID  # n_models = 0
    assert lib().ppca_mix_sparse_component_llks(ctx.handle, sp._sh, arr, 0, ptr(out)) == INVALID
    assert lib().ppca_mix_sparse_em_step(ctx.handle, sp._sh, arr, ptr(lw), 0, None, arr, ptr(lw_out), None) == INVALID
    assert lib().ppca_mix_sparse_predict(ctx.handle, sp._sh, arr, ptr(lw), 0, ptr(query[0]), ptr(query[1]), None, None) == INVALID
    h = C.c_void_p()
    assert lib().ppca_model_alloc(ctx.handle, 9, 3, C.byref(h)) == 0
    try:
        # an output that is its component's input, for either component (the dense step's check: per component)
        for pair in ((h, devs[1].h), (devs[0].h, h)):
            aliased = (C.c_void_p * 2)(*pair)
            assert lib().ppca_mix_sparse_em_step(ctx.handle, sp._sh, arr, ptr(lw), 2, None, aliased, ptr(lw_out), None) == INVALID, pair
            assert b"alias" in lib().ppca_last_error()
    finally:
        lib().ppca_model_free(h)

    with pytest.raises(ValueError, match="k-means takes a dense Dataset"):
        P.PPCAMix.init(2, 3, sp, seed=1, method="kmeans")
    with pytest.raises(TypeError):
        good.smooth(sp)
