"""Every EM and output path under STRUCTURED missing-data patterns (tests/mask_patterns.py) against the oracle.

Every other GPU test masks i.i.d. Bernoulli, so every mask word of every row is a random mix of bits, every tile has live rows and every
row has far more observed entries than states.  Here n = 293 everywhere (nine full 32-row tiles and one of 5 rows) and every pattern of
mask_patterns.NAMES runs through

  path                                                   (d, k)
  em9 + eight-wave llk sweep + pass_kernel               (256, 10), (255, 7), (64, 1)
  em16 two-kernel pass (outputs on the split pipeline)   (256, 11), (200, 16)
  split pipeline: lane / batched blocked / MFMA solver   (300, 4) / (70, 20) / (150, 80)

as statistics (ppca_stats_raw block by block, un-weighted and weighted, un-weighted observed counts EXACT), every output pass, and one
weighted EM step; the fused and two-kernel shapes on ONE workgroup walking all ten tiles in order (so that `tile_blocks` and
`thin_tiles` are "first tile empty", "whole 64-row group empty", "few live rows under the floor exponent") and on the full grid (every
tile some workgroup's first); the split pipeline also in five chunks of 64 rows (PPCA_GEN_CHUNK=64: chunk 1 of `tile_blocks` has no
observed entry, the last has 37 rows).  Then the mixture (mix_llk8_kernel, the gathered em9 instantiation) and the pairwise moments,
which read the mask through kernels of their own.

Tolerances are those of the files each shape is already tested in (tests/test_gpu_steady_state.py: 1e-9 statistics, 1e-10
log-likelihoods, 1e-9 outputs; tests/test_gpu_split_steady_state.py: 1e-8 statistics, 1e-9 log-likelihoods, 1e-7 states and
covariances, 1e-8 reconstructions); the two CPU restatements of the reference agree to <= 3e-12 on every pattern
(tests/test_mask_patterns_host.py).  The oracle's results are computed once per (shape, pattern) and shared; nobody writes to them.
Every check prints its figures, the rescale counters and the guards' verdicts before it asserts."""
import ctypes as C

import numpy as np
import pytest

import mask_patterns as MP
import moments_restatement as MR

pytestmark = pytest.mark.gpu

N = 293
TILES = (N + 31) // 32
FUSED = [(256, 10), (255, 7), (64, 1)]
TWO_KERNEL = [(256, 11), (200, 16)]
LANE, LANE_WIDE, SOLVE4, MFMA = 1, 2, 3, 4  # ppca_generic_trace::solver
SPLIT = {(300, 4): (LANE, LANE_WIDE), (70, 20): (SOLVE4,), (150, 80): (MFMA,)}
CHUNKED = ("tile_blocks", "thin_tiles")
RTOL = 1e-5  # tests/test_gpu_parity.py::test_mixture_against_oracle

# (d, k, pattern, chunk rows of the split pipeline or 0)
CASES = [(d, k, name, 0) for d, k in FUSED + TWO_KERNEL + list(SPLIT) for name in MP.NAMES]
CASES += [(d, k, name, 64) for d, k in SPLIT for name in CHUNKED]
IDS = ["d%d-k%d-%s%s" % (d, k, name, "-chunk%d" % ch if ch else "") for d, k, name, ch in CASES]


def _tols(d, k):
    """stats, llk, states / covariances / diagonals, reconstructions, of the file the shape is already tested in"""
    if (d, k) in FUSED:
        return dict(stats=1e-9, llk=1e-10, state=1e-9, recon=1e-9)
    if (d, k) in TWO_KERNEL:
        return dict(stats=1e-9, llk=1e-9, state=1e-7, recon=1e-8)
    return dict(stats=1e-8, llk=1e-9, state=1e-7, recon=1e-8)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@pytest.fixture()
def ctx(P):
    from ppca_rs_amd import _lib

    c = _lib.default_context()
    c.set_grid_limit(0)
    c.set_heavy_rows(8)
    c.debug_counters(reset=True)
    yield c
    c.set_grid_limit(0)
    c.set_heavy_rows(8)


@pytest.fixture()
def chunked(monkeypatch):
    def set_chunk(rows):
        if rows:
            monkeypatch.setenv("PPCA_GEN_CHUNK", str(rows))  # (read per call: ppca_generic.hip, gen_chunk)

    return set_chunk


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _blocks(d, k):
    kp = k * (k + 1) // 2
    b = [0, d * k, d * k + d * kp, 2 * d * k + d * kp, 2 * d * k + d * kp + d, 2 * d * k + d * kp + 2 * d]
    return list(zip(["cross", "S", "U", "sumx", "totals", "scalars"], b, b[1:] + [b[-1] + 8]))


_REF = {}


def _ref(oracle, d, k, name):
    """The case and everything the oracle says about it, once per (shape, pattern)."""
    key = (d, k, name)
    if key not in _REF:
        x, w, (s, c, mu), mask = MP.case(oracle, N, d, k, name, 1000 + 7 * d + k)
        r = dict(x=x, w=w, model=(s, c, mu), mask=mask)
        r["stats"] = {False: oracle.stats(x, s, c, mu), True: oracle.stats(x, s, c, mu, w)}
        r["llks"], r["llk_w"] = oracle.llks(x, s, c, mu), oracle.llk(x, s, c, mu, w)
        r["states"], r["covs"] = oracle.infer(x, s, c, mu)
        for mode in ("smooth", "extrapolate"):
            r[mode] = oracle.reconstruct(x, s, c, mu, mode)
            r["diag_" + mode] = oracle.covariance_diagonal(x, s, c, mu, mode)
        r["iterate_w"] = oracle.iterate(x, s, c, mu, w)
        for v in r.values():
            for a in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _stats_raw(ctx, ds, m):
    from ppca_rs_amd import _lib

    got = np.empty(_lib.lib().ppca_stats_len(m.output_size, m.state_size))
    _lib.check(_lib.lib().ppca_stats_raw(ctx.handle, ds._h, m._device(ctx).h, _lib.ptr(got)))
    return got


def _assert_stats(got, want, d, k, tol, mask, weighted, tag):
    errs = {name: _rel(got[a:b], want[a:b]) for name, a, b in _blocks(d, k)}
    print("stats", tag, " ".join("%s %.1e" % kv for kv in errs.items()), "(bound %.0e)" % tol)
    if not weighted:  # the observed counts are integers: exact
        (a, b), = [(a, b) for name, a, b in _blocks(d, k) if name == "totals"]
        assert np.array_equal(got[a:b], mask.sum(0).astype(np.float64)), ("totals", tag, np.flatnonzero(got[a:b] != mask.sum(0))[:8])
    for name, err in errs.items():
        assert err < tol, (name, err) + tuple(tag)


def _check_trace(t, d, k, chunk):
    """the dispatch record of a pass through the split pipeline: the solver the shape is here for, the chunks asked for"""
    assert t["valid"] == 1 and (t["d"], t["k"], t["n"]) == (d, k, N), t
    assert t["solver"] in SPLIT[(d, k)], ("another solver", d, k, t["solver"])
    assert t["chunks"] == (-(-N // chunk) if chunk else 1), ("chunks", t["chunks"])


@pytest.mark.parametrize("d,k,name,chunk", CASES, ids=IDS)
def test_statistics(P, oracle, ctx, chunked, d, k, name, chunk):
    """ppca_stats_raw block by block, un-weighted and weighted; the un-weighted observed counts exactly."""
    r = _ref(oracle, d, k, name)
    s, c, mu = r["model"]
    m = P.PPCAModel(s, c, mu)
    tol = _tols(d, k)["stats"]
    chunked(chunk)
    if (d, k) in SPLIT:
        for weighted in (False, True):
            got = _stats_raw(ctx, P.Dataset(r["x"], r["w"] if weighted else None), m)
            t = ctx.generic_trace()
            print("trace", (d, k, name, chunk), {a: t[a] for a in ("solver", "solver_nb", "chunks", "int8", "fused16", "wdigits_first", "wdigits_predicted")})
            assert t["em"] == 1 and t["fused16"] == 0, t
            _check_trace(t, d, k, chunk)
            _assert_stats(got, r["stats"][weighted], d, k, tol, r["mask"], weighted, (d, k, name, chunk, weighted))
        return
    base = 0 if k <= 10 else 4
    for cap in (1, 0):  # one workgroup walks all ten tiles in order; the full grid: every tile is some workgroup's first
        ctx.set_grid_limit(cap)
        for weighted in (False, True):
            ctx.debug_counters(reset=True)
            got = _stats_raw(ctx, P.Dataset(r["x"], r["w"] if weighted else None), m)
            cnt = ctx.debug_counters()
            tag = (d, k, name, "limit %d" % cap, "weighted" if weighted else "plain")
            print("counters", tag, "rescales %d flushes %d tiles %d" % tuple(cnt[base:base + 3]),
                  "guard (gram, stats) %s fallback (mode, workgroups, rows) %s" % (ctx.last_guard(), ctx.last_fallback()[:3]) if k <= 10
                  else "workgroups on the fp64 statistics %d" % cnt[7])
            if cap == 1:
                assert cnt[base + 2] == TILES, ("tiles walked by the one workgroup", cnt)
            if k >= 11:
                t = ctx.generic_trace()
                assert t["valid"] == 1 and t["em"] == 1 and t["fused16"] == 1, t
            _assert_stats(got, r["stats"][weighted], d, k, tol, r["mask"], weighted, tag)


@pytest.mark.parametrize("d,k,name,chunk", CASES, ids=IDS)
def test_output_passes(P, oracle, ctx, chunked, d, k, name, chunk):
    """llks, llk (weighted), states, covariances, smooth, extrapolate and both covariance diagonals; the all-masked rows exactly."""
    from ppca_rs_amd import _lib

    r = _ref(oracle, d, k, name)
    x, w, (s, c, mu), mask = r["x"], r["w"], r["model"], r["mask"]
    tol = _tols(d, k)
    tag = (d, k, name, chunk)
    m, ds = P.PPCAModel(s, c, mu), P.Dataset(x)
    dead = ~mask.any(1)
    chunked(chunk)

    def seen(what):
        if (d, k) in FUSED:
            return
        t = ctx.generic_trace()  # (k = 11..16: every pass but the EM pass is the split pipeline's)
        assert t["em"] == 0, (what, t)
        if (d, k) in SPLIT:
            _check_trace(t, d, k, chunk)
        else:
            assert t["valid"] == 1 and t["solver"] in (LANE, LANE_WIDE) and t["n"] == N, (what, t)

    errs = {}
    llks = m.llks(ds)
    seen("llks")
    errs["llks"] = _rel(llks, r["llks"])
    got = m.llk(P.Dataset(x, w))
    seen("llk")
    errs["llk"] = abs(got - r["llk_w"]) / abs(r["llk_w"])
    inf = m.infer(ds)
    seen("infer")
    states, covs = inf.states(), np.array(inf.covariances())
    errs["states"], errs["covariances"] = _rel(states, r["states"]), _rel(covs, r["covs"])
    sm = m.smooth(ds).numpy()
    seen("smooth")
    errs["smooth"] = _rel(sm, r["smooth"])
    ex = m.extrapolate(ds).numpy()
    seen("extrapolate")
    errs["extrapolate"] = _rel(ex, r["extrapolate"])
    diag = {}
    for mode, what in ((0, "smooth"), (1, "extrapolate")):
        h = C.c_void_p()
        _lib.check(_lib.lib().ppca_covariance_diagonal(ctx.handle, ds._h, m._device(ctx).h, mode, C.byref(h)))
        seen("diag_" + what)
        diag[what] = P.Dataset._wrap(h, ctx).numpy()
        errs["diag_" + what] = _rel(diag[what], r["diag_" + what])
    print("post", tag, " ".join("%s %.1e" % kv for kv in errs.items()), "all-masked rows %d" % dead.sum())
    assert errs["llks"] < tol["llk"] and errs["llk"] < tol["llk"], (tag, errs)
    assert max(errs["states"], errs["covariances"], errs["diag_smooth"], errs["diag_extrapolate"]) < tol["state"], (tag, errs)
    assert max(errs["smooth"], errs["extrapolate"]) < tol["recon"], (tag, errs)
    assert np.array_equal(ex[mask], x[mask]), tag  # observed entries: bit for bit
    assert np.array_equal(diag["extrapolate"][mask], np.zeros(mask.sum())), tag
    if dead.any():  # nothing observed: llk 0, posterior N(0, I), the mean reconstructed -- z is exactly 0, so C z + mu is mu in any order
        assert np.array_equal(llks[dead], np.zeros(dead.sum())), tag
        assert np.array_equal(states[dead], np.zeros((dead.sum(), k))), tag
        assert np.abs(covs[dead] - np.eye(k)).max() <= 1e-15, tag
        assert np.array_equal(sm[dead], np.tile(mu, (dead.sum(), 1))), tag
        assert np.array_equal(ex[dead], np.tile(mu, (dead.sum(), 1))), tag


@pytest.mark.parametrize("d,k,name,chunk", CASES, ids=IDS)
def test_one_em_step(P, oracle, ctx, chunked, d, k, name, chunk):
    """iterate_with_llk, weighted, against oracle.iterate at 1e-8; a column nobody observes keeps its row of C and its mean bit for bit
    (ppca_model.rs:313-321, :373-377; tests/test_gpu_parity.py::test_edge_cases at d = 16)."""
    r = _ref(oracle, d, k, name)
    x, w, (s, c, mu), mask = r["x"], r["w"], r["model"], r["mask"]
    s1, c1, m1 = r["iterate_w"]
    chunked(chunk)
    new, llk = P.PPCAModel(s, c, mu).iterate_with_llk(P.Dataset(x, w))
    if (d, k) in SPLIT:
        _check_trace(ctx.generic_trace(), d, k, chunk)
    errs = dict(C=_rel(new.transform, c1), mean=_rel(new.mean, m1), sigma=abs(new.isotropic_noise - s1) / s1, llk=abs(llk - r["llk_w"]) / abs(r["llk_w"]))
    never = ~mask.any(0)
    print("em step", (d, k, name, chunk), " ".join("%s %.1e" % kv for kv in errs.items()), "columns never observed %d" % never.sum(),
          "guard %s" % (ctx.last_guard(),) if (d, k) in FUSED else "")
    assert max(errs.values()) < 1e-8, errs
    if name == "column_once":
        assert never[1] and not never[list(MP.once_columns(d))].any()
    assert np.array_equal(new.transform[never], c[never]) and np.array_equal(new.mean[never], mu[never])


# --------------------------------------------------------------------------- the mixture
_MIX = {}


def _mix_case(oracle, name):
    """Three components at (256, 10): rows from three shifted synth sets under one pattern, the models near the three truths (so that
    most rows belong to one component and the rows with few or no observed entries to all three)."""
    if name not in _MIX:
        d, k, nm = 256, 10, 3
        rng = np.random.default_rng(77)
        sizes = [N // nm + (i < N % nm) for i in range(nm)]
        parts, cs, ms = [], [], []
        for i, sz in enumerate(sizes):
            xx, ct, mt = oracle.synth(sz, d, k, 0.0, 300 + i, mean_scale=3.0)
            parts.append(xx)
            cs.append(0.7 * ct + 0.2 * rng.standard_normal((d, k)))
            ms.append(mt + 0.2 * rng.standard_normal(d))
        x = np.concatenate(parts)
        mask = MP.patterns(N, d, k, 300)[name]
        x[~mask] = np.nan
        sig, cs, ms, lw = np.array([1.0, 1.2, 0.9]), np.array(cs), np.array(ms), np.log(np.array([0.3, 0.3, 0.4]))
        r = dict(x=x, mask=mask, model=(sig, cs, ms, lw), llks=oracle.mix_llks(x, sig, cs, ms, lw),
                 cluster=oracle.mix_infer_cluster(x, sig, cs, ms, lw), iterate=oracle.mix_iterate(x, sig, cs, ms, lw))
        _MIX[name] = r
    return _MIX[name]


@pytest.mark.parametrize("name", MP.NAMES)
def test_mixture(P, oracle, ctx, name):
    """mix_llk8_kernel and the gathered em9 instantiation (the row gather changes which rows share a tile): llks and log-posteriors at
    1e-8, one mixture EM step at the 1e-5 of tests/test_gpu_parity.py::test_mixture_against_oracle."""
    r = _mix_case(oracle, name)
    x, (sig, cs, ms, lw) = r["x"], r["model"]
    ds = P.Dataset(x)
    mix = P.PPCAMix([P.PPCAModel(sig[i], cs[i], ms[i]) for i in range(len(sig))], lw)
    errs = dict(llks=_rel(mix.llks(ds), r["llks"]), cluster=_rel(mix.infer_cluster(ds), r["cluster"]))
    new, llk = mix.iterate_with_llk(ds)
    s1, c1, m1, lw1 = r["iterate"]
    errs["llk"] = abs(llk - r["llks"].sum()) / abs(r["llks"].sum())
    errs["sigma"] = max(abs(mdl.isotropic_noise - s1[i]) / s1[i] for i, mdl in enumerate(new.models))
    errs["C"] = max(_rel(mdl.transform, c1[i]) for i, mdl in enumerate(new.models))
    errs["mean"] = max(_rel(mdl.mean, m1[i]) for i, mdl in enumerate(new.models))
    errs["log_weights"] = _rel(new.log_weights, lw1)
    print("mixture", name, " ".join("%s %.1e" % kv for kv in errs.items()), "posterior weights per component", np.exp(r["cluster"]).sum(0).round(1),
          "guard", ctx.last_guard())
    assert errs["llks"] < 1e-8 and errs["cluster"] < 1e-8 and errs["llk"] < 1e-8, errs
    assert max(errs["sigma"], errs["C"], errs["mean"], errs["log_weights"]) < RTOL, errs


# --------------------------------------------------------------------------- the pairwise moments
@pytest.mark.parametrize("name", MP.NAMES)
@pytest.mark.parametrize("d", [130, 256])
def test_pairwise_moments(P, oracle, d, name):
    """Dataset.pairwise_moments(cross=True) against tests/moments_restatement.py at the 1e-11 of
    tests/test_gpu_pairwise_moments.py::test_pass_against_restatement, about an arbitrary centre as there (about the weighted column
    means the cross matrix of two columns observed in the same rows -- every pair under `full` -- is zero but for its rounding, and
    a bound relative to the largest entry says nothing); the un-weighted pair counts are M^T M exactly."""
    x, w, _, mask = MP.case(oracle, N, d, 4, name, 2000 + d)
    center = 3.0 * np.random.default_rng(d).standard_normal(d)
    for weights in (None, w):
        got = P.Dataset(np.array(x), None if weights is None else np.array(weights)).pairwise_moments(center, cross=True)
        errs = dict(zip(("sums", "counts", "cross"), (_rel(g, r) for g, r in zip((got.sums, got.counts, got.cross), MR.moments(x, weights, center)))))
        print("moments", (d, name, "plain" if weights is None else "weighted"), " ".join("%s %.1e" % kv for kv in errs.items()))
        assert max(errs.values()) < 1e-11, errs
        if weights is None:
            mi = mask.astype(np.int64)
            assert np.array_equal(got.counts, (mi.T @ mi).astype(np.float64))
        assert np.array_equal(got.sums, got.sums.T) and np.array_equal(got.counts, got.counts.T)
