"""The inventory of passes of tests/test_gpu_recycled_memory.py and tests/test_recycled_memory_host.py.  No test lives
here.

One Entry per pass (or per small family of passes that share their inputs): `run(P, ctx)` builds its datasets and models on the given
private context from the shared read-only cases of the other case modules, runs the passes, and returns a dict of arrays / scalars --
the outputs, and the diagnostics that read context state after the pass where the pass defines them.  Every handle `run` creates is
released when it returns, so the blocks go back to the context's cache: that is what the next run draws from, dirtied or not.
`symbols` are the C-ABI entry points the run drives (tests/test_recycled_memory_host.py holds the table of ppca_rs_amd/_lib.py against
them).

Which diagnostic a pass defines:
  last_guard / last_fallback   the fused EM pass (d <= 256, k <= 10) and the multi-component mixture step: include/ppca_hip.h says "of
                               the most recent FUSED EM pass"; the two-kernel pass and the split pipeline file no verdict there
  last_llk (ppca_em_last_llk)  every EM step that writes the context's statistics buffer: the plain steps (dense, row-compressed) leave
                               the place of their llk there; the mixture, factor-analysis and Student-t steps overwrite the buffer
                               and withdraw it (then the call fails: recorded as None).  Not the known-precision step, which has
                               scratch of its own: after it the call still reports the last plain step, as include/ppca_hip.h says
  trace                        every pass through the split pipeline (ppca_generic_last_trace); the two-kernel EM pass marks fused16
  rows_used                    every mixture step (ppca_mix_last_rows_used)

Engines by shape (the gates of ppca_path_kind, ppca_generic.hip's launch_solve and state_size_cases' table): `engine_of`.
"""
import ctypes as C
import functools

import numpy as np

import hppca_restatement as HR  # noqa: F401  (state_size_cases builds on it)
import sparse_cases as SC
import sparse_fa_cases as SFC
import sparse_mix_cases as SMC
import sparse_t_cases as STC
import state_size_cases as S

N_DENSE = 200  # rows of the dense engine cases: seven 32-sample tiles, the last one partial
TILING = dict(block_rows=64, segment=8)  # sparse_fa_cases.SWEEP_TILING: three row blocks and cut columns at (150, 300)
SPARSE_KS = (3, 16)
NU = 4.0

# (d, k) -> engine, the smallest shapes of the issue
ENGINE_SHAPES = [(200, 4, "em9"), (256, 10, "em9"), (200, 13, "em16"), (270, 7, "lane"), (70, 20, "solve4"), (90, 65, "mfma"),
                 (40, 0, "em9")]
VARIANT_SHAPES = [(256, 10), (200, 16)]  # the guard-tripping model, the outlier row and the prior


def engine_of(d, k, path_kind):
    """The engine the EM pass of a (d, k) model runs on; path_kind = ppca_path_kind(d, k).
    1: the fused eight-wave pass (d <= 256, k <= 10; k = 0 runs as one zero column).  0: the split pipeline -- its EM pass is the
    two-kernel pass for d <= 256, 11 <= k <= 16, and its per-sample solver goes by k: a lane per sample up to 16, the batched blocked
    solver (solve4) for 17 .. 64, a sample per wave on the MFMA beyond."""
    if path_kind == 1:
        return "em9"
    assert path_kind == 0, (d, k, path_kind)
    if k <= 16:
        return "em16" if d <= 256 and k >= 11 else "lane"
    return "solve4" if k <= 64 else "mfma"


SOLVER_OF = dict(lane=(1, 2), em16=(1, 2), solve4=(3,), mfma=(4,))  # ppca_generic_trace.solver of the output passes


class Entry:
    def __init__(self, name, run, symbols, *, shape=None, engine=None, oracle=None, exempt_line=None, biggest=0):
        self.name, self.run, self.symbols = name, run, tuple(symbols)
        self.shape, self.engine = shape, engine  # (d, k) and the engine the name claims, where it claims one
        self.oracle = oracle  # oracle(oracle_module, result) -> asserts, for the entries an existing test holds to the oracle
        self.exempt_line = exempt_line  # "file:line" that makes the bits depend on something besides the inputs (none does today)
        self.biggest = biggest  # bytes of the entry's largest device output (a floor for what dirty_scratch must have filled)

    def __repr__(self):
        return self.name


ENTRIES = []


def _add(name, symbols, **kw):
    def deco(fn):
        ENTRIES.append(Entry(name, fn, symbols, **kw))
        return fn
    return deco


def by_name(name):
    return next(e for e in ENTRIES if e.name == name)


# ------------------------------------------------------------------ helpers
def _L():
    from ppca_rs_amd import _lib

    return _lib


def last_llk(ctx):
    L = _L()
    v = C.c_double(0.0)
    rc = L.lib().ppca_em_last_llk(ctx.handle, C.byref(v))
    return float(v.value) if rc == 0 else None


def fallback(ctx):
    return ctx.last_fallback()[:3]  # (the fourth value is a time)


def rows_used(ctx, nm):
    L = _L()
    out = (C.c_int64 * nm)()
    L.check(L.lib().ppca_mix_last_rows_used(ctx.handle, out, nm))
    return [int(v) for v in out]


def model_out(m, tag=""):
    return {tag + "sigma": m.isotropic_noise, tag + "C": m.transform, tag + "mean": m.mean}


def mix_out(mix, tag=""):
    out = {tag + "logw": mix.log_weights}
    for c, m in enumerate(mix.models):
        out.update(model_out(m, "%sm%d_" % (tag, c)))
    return out


def score_out(h, tag):
    return {tag + "cols": h._cols, tag + "n_entries": h.n_entries, tag + "n_rows": h.n_rows, tag + "llks": h._llks}


def stats_raw(ds, m):
    L = _L()
    out = np.empty(int(L.lib().ppca_stats_len(m.output_size, max(m.state_size, 1))))
    L.check(L.lib().ppca_stats_raw(ds._ctx.handle, ds._h, m._device(ds._ctx).h, L.ptr(out)))
    return out


def cov_diag(P, ds, m, mode):
    L = _L()
    h = C.c_void_p()
    L.check(L.lib().ppca_covariance_diagonal(ds._ctx.handle, ds._h, m._device(ds._ctx).h, mode, C.byref(h)))
    return P.Dataset._wrap(h, ds._ctx).numpy()


class DevBuf:
    """n doubles of device memory that a live Dataset handle owns (never in the cache, never dirtied): the stats_dev / u_dev / out_dev
    arguments of the entry points that write device memory of the caller."""

    def __init__(self, P, ctx, n):
        self.ds = P.Dataset(np.zeros((1, max(int(n), 1))), ctx=ctx)
        self.ptr = C.c_void_p(_L().lib().ppca_dataset_device_x(self.ds._h))

    def at(self, doubles):
        return C.c_void_p(self.ptr.value + 8 * int(doubles))

    def numpy(self):
        return self.ds.numpy()[0]


@functools.lru_cache(maxsize=None)
def dense(d, k, variant="plain"):
    """state_size_cases.dense_case at N_DENSE rows (k = 0: the data of k = 1 under a model without a transform).
    variant "guard": row 0 of C times 1e8, the model of test_last_guard_after_a_larger_model whose Gram guard trips;
    "outlier": row 37 of the data times 1e6, which the guard of the int8 mask-side statistics answers with its fp64 second stage."""
    x, w, (s, c, mu) = S.dense_case(N_DENSE, d, max(k, 1))
    if k == 0:
        c = np.zeros((d, 0))
    if variant == "guard":
        c = c.copy()
        c[0] *= 1e8
    if variant == "outlier":
        x = x.copy()
        x[37] *= 1e6
    for a in (x, c):
        a.setflags(write=False)
    return x, w, (s, c, mu)


def prior_of(P, d):
    rng = np.random.default_rng(50 + d)
    return (P.Prior().with_isotropic_noise_prior(2.0, 3.0).with_transformation_precision(0.7)
            .with_mean_prior(0.1 * rng.standard_normal(d), np.diag(rng.uniform(0.5, 2.0, d))))


# ------------------------------------------------------------------ the engines behind PPCAModel
ENGINE_SYMBOLS = ("ppca_dataset_from_host", "ppca_model_create", "ppca_model_alloc", "ppca_model_download", "ppca_em_step",
                  "ppca_em_last_llk", "ppca_stats_raw", "ppca_llk", "ppca_llks_dev", "ppca_infer", "ppca_reconstruct",
                  "ppca_covariance_diagonal", "ppca_dataset_to_host", "ppca_em_last_guard", "ppca_em_last_fallback",
                  "ppca_generic_last_trace", "ppca_gram_engine")


def _engine_run(d, k, engine, P, ctx):
    L = _L()
    x, w, (s, c, mu) = dense(d, k)
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    n = len(ds)
    out = {}
    new, llk = m.iterate_with_llk(ds)
    out.update(model_out(new, "it_"), it_llk=llk, last_llk=last_llk(ctx))
    if engine == "em9":
        out.update(guard=ctx.last_guard(), fallback=fallback(ctx))
    else:
        out["trace_em"] = ctx.generic_trace()
    out["stats"] = stats_raw(ds, m)
    out["llks"], out["llk"] = m.llks(ds), m.llk(ds)
    dev = DevBuf(P, ctx, n)
    L.check(L.lib().ppca_llks_dev(ctx.handle, ds._h, m._device(ctx).h, dev.ptr))
    out["llks_dev"] = dev.numpy()
    inf = m.infer(ds)
    out["states"], out["covs"] = inf._states, inf._covs
    out["smooth"], out["extrapolate"] = m.smooth(ds).numpy(), m.extrapolate(ds).numpy()
    out["diag_smooth"], out["diag_extrapolate"] = cov_diag(P, ds, m, 0), cov_diag(P, ds, m, 1)
    if engine != "em9":
        out["trace_out"] = ctx.generic_trace()
    eng = C.c_int32(-1)
    L.check(L.lib().ppca_gram_engine(ctx.handle, m._device(ctx).h, C.byref(eng)))
    out["gram_engine"] = int(eng.value)
    return out


def _engine_oracle(d, k):
    """The comparisons and tolerances of tests/test_gpu_parity.py::test_generic_pipeline_matches_oracle (its shapes are these engines'),
    with its RTOL = 1e-5 for the step; k = 0 against the same oracle under one zero column."""
    def check(o, r):
        x, w, (s, c, mu) = dense(d, k)
        c1 = c if k else np.zeros((d, 1))

        def rel(a, b):
            a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
            return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)

        want = o.stats(x, s, c1, mu, w)
        kk = max(k, 1)
        kp = kk * (kk + 1) // 2
        b = [0, d * kk, d * kk + d * kp, 2 * d * kk + d * kp, 2 * d * kk + d * kp + d, 2 * d * kk + d * kp + 2 * d, want.size]
        for name, lo, hi in zip(["cross", "S", "U", "sumx", "totals", "scalars"], b[:-1], b[1:]):
            assert rel(r["stats"][lo:hi], want[lo:hi]) < 1e-8, name
        assert rel(r["llks"], o.llks(x, s, c1, mu)) < 1e-9 and rel(r["llks_dev"], o.llks(x, s, c1, mu)) < 1e-9
        want_llk = o.llk(x, s, c1, mu, w)
        assert abs(r["llk"] - want_llk) < 1e-9 * abs(want_llk)
        assert abs(r["it_llk"] - want_llk) < 1e-5 * 1e-3 * abs(want_llk) and r["last_llk"] == r["it_llk"]
        if k:
            st, cv = o.infer(x, s, c, mu)
            assert rel(r["states"], st) < 1e-7 and rel(r["covs"], cv) < 1e-7
            for mode in ("smooth", "extrapolate"):
                assert rel(r["diag_" + mode], o.covariance_diagonal(x, s, c, mu, mode)) < 1e-7, mode
        assert rel(r["smooth"], o.reconstruct(x, s, c1, mu, "smooth")) < 1e-8
        assert rel(r["extrapolate"], o.reconstruct(x, s, c1, mu, "extrapolate")) < 1e-8
        s1, cn, m1 = o.iterate(x, s, c1, mu, w)
        assert abs(r["it_sigma"] - s1) < 1e-5 * s1 and rel(r["it_mean"], m1) < 1e-5
        if k:
            assert rel(r["it_C"], cn) < 1e-5
    return check


for _d, _k, _e in ENGINE_SHAPES:
    _add("engine_%s_%dx%d" % (_e, _d, _k), ENGINE_SYMBOLS, shape=(_d, _k), engine=_e, oracle=_engine_oracle(_d, _k),
         biggest=8 * N_DENSE * max(_d, _k * _k))(functools.partial(_engine_run, _d, _k, _e))


def _variant_run(d, k, variant, P, ctx):
    x, w, (s, c, mu) = dense(d, k, variant if variant != "prior" else "plain")
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    out = {}
    if variant == "prior":
        new = m.iterate_with_prior(ds, prior_of(P, d))
        llk = None
    elif variant == "outlier":
        # By default the eight-wave pass sends a few such rows round its fixed-point form and the second stage has nothing to do;
        # ppca_ctx_set_heavy_rows(0) puts the guard of the statistics, and the fp64 second stage behind it, back in charge (the
        # two-kernel pass has only that answer).  The counters of the int8 contraction are the library's, reset here.
        ctx.set_heavy_rows(0)
        try:
            ctx.debug_counters(reset=True)
            new, llk = m.iterate_with_llk(ds)
            out["counters"] = ctx.debug_counters(reset=True)
        finally:
            ctx.set_heavy_rows(8)
    else:
        new, llk = m.iterate_with_llk(ds)
    out.update(model_out(new, "it_"), it_llk=llk, last_llk=last_llk(ctx))
    if k <= 10:
        out.update(guard=ctx.last_guard(), fallback=fallback(ctx))
    else:
        out["trace_em"] = ctx.generic_trace()
    out["llks"] = m.llks(ds)  # (a guard-tripping model: the llk sweep's fp64 instantiation)
    out["smooth"] = m.smooth(ds).numpy()
    L = _L()
    eng = C.c_int32(-1)
    L.check(L.lib().ppca_gram_engine(ctx.handle, m._device(ctx).h, C.byref(eng)))
    out["gram_engine"] = int(eng.value)
    return out


for _d, _k in VARIANT_SHAPES:
    for _v in ("guard", "outlier", "prior"):
        _add("step_%s_%dx%d" % (_v, _d, _k), ("ppca_em_step", "ppca_llk", "ppca_reconstruct", "ppca_em_last_guard", "ppca_em_last_fallback",
                                              "ppca_gram_engine", "ppca_ctx_set_heavy_rows", "ppca_debug_counters"),
             shape=(_d, _k), engine="em9" if _k <= 10 else "em16", biggest=8 * N_DENSE * _d)(functools.partial(_variant_run, _d, _k, _v))


@_add("accumulate_finalize_256x10", ("ppca_em_accumulate", "ppca_em_finalize", "ppca_dataset_device_x"), shape=(256, 10), engine="em9",
      biggest=8 * 256 * 87)
def _accumulate_finalize(P, ctx):
    """The two halves of the step as the sharded hosts call them: statistics into device memory of the caller, then the finalisation."""
    L = _L()
    x, w, (s, c, mu) = dense(256, 10)
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    stats = DevBuf(P, ctx, L.lib().ppca_stats_len(256, 10))
    L.check(L.lib().ppca_em_accumulate(ctx.handle, ds._h, m._device(ctx).h, stats.ptr))
    h = C.c_void_p()
    L.check(L.lib().ppca_model_alloc(ctx.handle, 256, 10, C.byref(h)))
    from ppca_rs_amd import api

    dev = api._DevModel(h)
    L.check(L.lib().ppca_em_finalize(ctx.handle, m._device(ctx).h, stats.ptr, None, dev.h))
    new = P.PPCAModel._from_device(dev, ctx, 256, 10)
    return dict(stats=stats.numpy(), guard=ctx.last_guard(), fallback=fallback(ctx), **model_out(new, "it_"))


# ------------------------------------------------------------------ dataset plumbing and output passes
@_add("dataset_plumbing", ("ppca_dataset_generate", "ppca_dataset_with_weights", "ppca_dataset_slice", "ppca_dataset_concat",
                           "ppca_dataset_weights_to_host", "ppca_dataset_from_device", "ppca_dataset_scale_rows",
                           "ppca_dataset_scale_columns", "ppca_dataset_fill_masked", "ppca_dataset_column_moments_multi"),
      biggest=8 * 300 * 64)
def _plumbing(P, ctx):
    L = _L()
    rng = np.random.default_rng(3)
    truth = P.PPCAModel(0.3, rng.standard_normal((64, 5)), rng.standard_normal(64), ctx=ctx)
    gen = truth.sample(300, 0.3, seed=11, ctx=ctx)
    out = dict(generated=gen.numpy())
    rows = (C.c_int64 * 2)(5, 250)
    L.check(L.lib().ppca_dataset_scale_rows(gen._h, rows, 2, 4.0))
    out["scaled_rows"] = gen.numpy()
    w = rng.uniform(0.5, 2.0, 300)
    ww = gen.with_weights(w)
    parts = [ww._slice(0, 100), ww._slice(100, 200)]
    cat = P.Dataset.concat(parts[::-1])
    out.update(concat=cat.numpy(), concat_w=cat.weights())
    borrowed = P.Dataset.from_device(L.lib().ppca_dataset_device_x(cat._h), 300, 64, ctx=ctx, keepalive=cat)
    out["borrowed_empty"] = borrowed.empty_dimensions()
    a = rng.uniform(0.5, 2.0, 64)
    y, sums, rs = cat._scale_columns(a, rng.standard_normal(64), np.log(a), col_sums=True, row_sums=True)
    out.update(scaled=y.numpy(), col_sums=sums, row_sums=rs)
    out["filled"] = cat._fill_masked(y, a).numpy()
    out["moments_multi"] = cat._column_moments_multi(rng.uniform(0.0, 1.0, (3, 300)), a, rng.standard_normal((3, 64)))
    return out


@_add("mfma_probes", ("ppca_debug_mfma_probe", "ppca_debug_mfma_i8_probe"), biggest=3072)
def _probes(P, ctx):
    """The two unit probes of the MFMA lane maps: their operands and results pass through a block of the cache."""
    L = _L()
    rng = np.random.default_rng(8)
    a, b, out = rng.standard_normal((16, 4)), rng.standard_normal((4, 16)), np.empty((16, 16))
    L.check(L.lib().ppca_debug_mfma_probe(ctx.handle, L.ptr(a), L.ptr(b), L.ptr(out)))
    a8, b8 = rng.integers(-64, 64, (64, 16), dtype=np.int8), rng.integers(-64, 64, (64, 16), dtype=np.int8)
    o8 = np.empty((64, 4), dtype=np.int32)
    L.check(L.lib().ppca_debug_mfma_i8_probe(ctx.handle, L.ptr(a8), L.ptr(b8), L.ptr(o8)))
    return dict(f64=out, i8=o8)


def _output_case():
    return dense(200, 4)


@_add("sample_posterior", ("ppca_posterior_sample",), biggest=8 * N_DENSE * 200)
def _sample_posterior(P, ctx):
    x, w, (s, c, mu) = _output_case()
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    return dict(draw=m.sample_posterior(ds, seed=7).numpy(), impute=m.sample_posterior(ds, seed=7, keep_observed=True, row_offset=3).numpy())


@_add("sample_posterior_split_70x20", ("ppca_posterior_sample",), shape=(70, 20), engine="solve4", biggest=8 * N_DENSE * 400)
def _sample_posterior_split(P, ctx):
    x, w, (s, c, mu) = dense(70, 20)
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    return dict(draw=m.sample_posterior(ds, seed=7).numpy(), impute=m.sample_posterior(ds, seed=7, keep_observed=True).numpy())


@_add("loo_predictive", ("ppca_loo_predictive",), biggest=8 * N_DENSE * 200)
def _loo(P, ctx):
    x, w, (s, c, mu) = _output_case()
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    full = m.loo_predictive(ds)
    return dict(mean=full.mean().numpy(), var=full.variance().numpy(), llks=full.llks(), llk=full.llk(), loo_llks=m.loo_llks(ds),
                loo_llk=m.loo_llk(ds))


@_add("holdout_kfold_score", ("ppca_dataset_holdout", "ppca_dataset_holdout_range", "ppca_heldout_score"), biggest=8 * N_DENSE * 200)
def _holdout(P, ctx):
    x, w, (s, c, mu) = _output_case()
    ds, m = P.Dataset(x, w, ctx=ctx), P.PPCAModel(s, c, mu, ctx=ctx)
    tr, he = ds.holdout(0.2, seed=5)
    out = dict(train=tr.numpy(), held=he.numpy(), counts=tr.holdout_counts, **score_out(m.heldout_score(tr, he), "score_"))
    for f, (t, h) in enumerate(ds.kfold(3, seed=9, row_offset=2)):
        out.update(score_out(m.heldout_score(t, h), "fold%d_" % f), **{"fold%d_counts" % f: t.holdout_counts})
    return out


@_add("column_passes", ("ppca_dataset_empty_dimensions", "ppca_dataset_scale_columns", "ppca_dataset_pairwise_moments"), biggest=8 * 200 * 200)
def _column_passes(P, ctx):
    x, w, _ = _output_case()
    x = x.copy()
    x[:, [3, 77, 199]] = np.nan
    ds = P.Dataset(x, w, ctx=ctx)
    tot, mean, var = ds.column_stats()
    pm = ds.pairwise_moments(cross=True)
    return dict(empty=ds.empty_dimensions(), tot=tot, mean=mean, var=var, center=pm._center, sums=pm._sums, counts=pm._counts,
                cross=pm._cross)


def _kmeans_run(K, P, ctx):
    x, w, _ = _output_case()
    ds = P.Dataset(x, w, ctx=ctx)
    centers, rows = ds._kmeans_seed(K, np.random.default_rng(K).random(K), None)
    out = dict(seed_centers=centers, seed_rows=rows)
    for it in range(2):
        step = ds.kmeans_step(centers, labels=True, distances=True)
        out.update({"labels%d" % it: step.labels, "dist%d" % it: step.distances, "totals%d" % it: step.totals, "sums%d" % it: step.sums,
                    "inertia%d" % it: step.inertia, "reads%d" % it: step.reads})
        centers = step.centers()
    km = ds.kmeans(K, n_iters=2, seed=K, scale="std")
    out.update(km_centers=km.centers, km_labels=km.labels, km_inertia=km.inertia, km_history=km.history, km_cw=km.cluster_weights)
    return out


for _K in (3, 8):
    _add("kmeans_K%d" % _K, ("ppca_dataset_kmeans_seed", "ppca_dataset_kmeans_step"), biggest=8 * N_DENSE)(functools.partial(_kmeans_run, _K))


# ------------------------------------------------------------------ mixtures
MIX_SYMBOLS = ("ppca_mix_em_step", "ppca_mix_last_rows_used", "ppca_mix_llk", "ppca_mix_reconstruct", "ppca_mix_posterior_sample",
               "ppca_mix_loo_predictive", "ppca_mix_heldout_score")


@functools.lru_cache(maxsize=None)
def mix_models(form):
    """state_size_cases.mix_case(4): three components of state size 4 (the multi-component form of the step), or -- "sizes" -- its
    first component and one of state size 20 (the step goes component by component: one fused, one through the split pipeline)."""
    x, w, (sig, cs, ms, lw) = S.mix_case(4)
    if form == "multi":
        return x, w, [(sig[c], cs[c], ms[c]) for c in range(3)], lw
    rng = np.random.default_rng(420)
    c20 = 0.3 * rng.standard_normal((x.shape[1], 20))
    c20.setflags(write=False)
    return x, w, [(sig[0], cs[0], ms[0]), (0.6, c20, ms[1])], np.log(np.array([0.6, 0.4]))


def _mix_run(form, P, ctx):
    x, w, comps, lw = mix_models(form)
    ds = P.Dataset(x, w, ctx=ctx)
    mix = P.PPCAMix([P.PPCAModel(s, c, mu, ctx=ctx) for s, c, mu in comps], lw)
    out = {}
    new, llk = mix.iterate_with_llk(ds)
    out.update(mix_out(new, "it_"), it_llk=llk, last_llk=last_llk(ctx), rows_used=rows_used(ctx, len(comps)))
    if form == "multi":
        out.update(guard=ctx.last_guard(), fallback=fallback(ctx))
    out["llks"], out["log_post"] = mix.llks(ds), mix.infer_cluster(ds)
    out["smooth"], out["extrapolate"] = mix.smooth(ds).numpy(), mix.extrapolate(ds).numpy()
    out["draw"] = mix.sample_posterior(ds, seed=13).numpy()
    out["impute"] = mix.sample_posterior(ds, seed=13, keep_observed=True).numpy()
    loo = mix.loo_predictive(ds)
    out.update(loo_mean=loo.mean().numpy(), loo_var=loo.variance().numpy(), loo_llks=loo.llks(), loo_llk=loo.llk())
    tr, he = ds.holdout(0.2, seed=5)
    out.update(score_out(mix.heldout_score(tr, he), "score_"))
    return out


def _mix_oracle(o, r):
    """tests/test_gpu_parity.py::test_mixture_against_oracle: llks 1e-9, log posteriors 1e-8, the step's llk 1e-8, the new mixture RTOL."""
    x, w, comps, lw = mix_models("multi")
    sig, cs, ms = np.array([c[0] for c in comps]), np.array([c[1] for c in comps]), np.array([c[2] for c in comps])

    def rel(a, b):
        return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)

    want_llks = o.mix_llks(x, sig, cs, ms, lw)
    assert rel(r["llks"], want_llks) < 1e-9
    assert rel(r["log_post"], o.mix_infer_cluster(x, sig, cs, ms, lw)) < 1e-8
    assert abs(r["it_llk"] - float(w @ want_llks)) < 1e-8 * abs(r["it_llk"])
    s1, c1, m1, lw1 = o.mix_iterate(x, sig, cs, ms, lw, w)
    for c in range(3):
        assert abs(r["it_m%d_sigma" % c] - s1[c]) < 1e-5 * s1[c]
        assert rel(r["it_m%d_C" % c], c1[c]) < 1e-5 and rel(r["it_m%d_mean" % c], m1[c]) < 1e-5
    assert rel(r["it_logw"], lw1) < 1e-5


_add("mix_multi_3x4", MIX_SYMBOLS, oracle=_mix_oracle, biggest=8 * 300 * 40)(functools.partial(_mix_run, "multi"))
_add("mix_sizes_4_20", MIX_SYMBOLS, biggest=8 * 300 * 40)(functools.partial(_mix_run, "sizes"))


@_add("mix_by_hand", ("ppca_mix_responsibilities_dev", "ppca_mix_component_stats", "ppca_vector_max_dev", "ppca_vector_sum_dev",
                      "ppca_vector_exp_shift_dev", "ppca_dataset_device_weights"), biggest=8 * 300 * 3)
def _mix_by_hand(P, ctx):
    """The pieces a host that shards the mixture itself calls (ppca_rs_amd/distributed.py)."""
    L = _L()
    x, w, comps, lw = mix_models("multi")
    n, d = x.shape
    ds = P.Dataset(x, w, ctx=ctx)
    mix = P.PPCAMix([P.PPCAModel(s, c, mu, ctx=ctx) for s, c, mu in comps], lw)
    devs, arr = mix._handles(ctx)
    u, lse, ex = DevBuf(P, ctx, 3 * n), DevBuf(P, ctx, n), DevBuf(P, ctx, n)
    lwn = np.ascontiguousarray(mix.log_weights)
    L.check(L.lib().ppca_mix_responsibilities_dev(ctx.handle, ds._h, arr, L.ptr(lwn), 3, u.ptr, lse.ptr))
    out = dict(u=u.numpy(), lse=lse.numpy())
    tot, mx = C.c_double(0.0), C.c_double(0.0)
    L.check(L.lib().ppca_vector_sum_dev(ctx.handle, lse.ptr, C.c_void_p(L.lib().ppca_dataset_device_weights(ds._h)), n, C.byref(tot)))
    out["llk"] = tot.value
    slen = int(L.lib().ppca_stats_len(d, 4))
    stats = DevBuf(P, ctx, slen)
    for c in range(3):
        L.check(L.lib().ppca_vector_max_dev(ctx.handle, u.at(c * n), n, C.byref(mx)))
        s, used = C.c_double(0.0), C.c_int64(0)
        L.check(L.lib().ppca_mix_component_stats(ctx.handle, ds._h, devs[c].h, u.at(c * n), mx.value, stats.ptr, C.byref(s), C.byref(used)))
        out.update({"max%d" % c: mx.value, "sum%d" % c: s.value, "used%d" % c: int(used.value), "stats%d" % c: stats.numpy()})
    L.check(L.lib().ppca_vector_exp_shift_dev(ctx.handle, u.ptr, mx.value, n, ex.ptr))
    out["exp_shift"] = ex.numpy()
    return out


def _fa_inputs():
    x, w, (sig, cs, ms, lw) = S.mix_case(4)
    noise = np.random.default_rng(44).uniform(0.5, 2.0, x.shape[1])
    return x, w, noise, cs, ms, lw


@_add("fa_model", ("ppca_fa_em_step", "ppca_dataset_scale_columns", "ppca_dataset_fill_masked"), biggest=8 * 300 * 40)
def _fa_model(P, ctx):
    x, w, noise, cs, ms, _ = _fa_inputs()
    ds, m = P.Dataset(x, w, ctx=ctx), P.FAModel(noise, cs[0], ms[0], ctx=ctx)
    new, llk = m.iterate_with_llk(ds, min_noise=1e-3)
    tr, he = ds.holdout(0.2, seed=5)
    return dict(it_noise=new.noise, it_C=new.transform, it_mean=new.mean, it_llk=llk, last_llk=last_llk(ctx), llks=m.llks(ds),
                smooth=m.smooth(ds).numpy(), extrapolate=m.extrapolate(ds).numpy(), **score_out(m.heldout_score(tr, he), "score_"))


@_add("fa_mix", ("ppca_famix_em_step", "ppca_dataset_column_moments_multi"), biggest=8 * 300 * 40)
def _fa_mix(P, ctx):
    x, w, noise, cs, ms, lw = _fa_inputs()
    ds, m = P.Dataset(x, w, ctx=ctx), P.FAMix(noise, cs, ms, lw, ctx=ctx)
    new, llk = m.iterate_with_llk(ds, min_noise=1e-3)
    tr, he = ds.holdout(0.2, seed=5)
    return dict(it_noise=new.noise, it_C=new.transforms, it_mean=new.means, it_logw=new.log_weights, it_llk=llk, last_llk=last_llk(ctx),
                llks=m.llks(ds), smooth=m.smooth(ds).numpy(), extrapolate=m.extrapolate(ds).numpy(),
                **score_out(m.heldout_score(tr, he), "score_"))


# ------------------------------------------------------------------ the Student-t and the known-precision models
def _t_run(d, P, ctx):
    x, w, (s, c, mu) = S.robust_case(d, 4)
    ds, m = P.Dataset(x, w, ctx=ctx), P.TPPCAModel(s, c, mu, NU, ctx=ctx)
    new, llk = m.iterate_with_llk(ds, estimate_dof=True)
    tr, he = ds.holdout(0.2, seed=5)
    return dict(it_dof=new.dof, it_llk=llk, last_llk=last_llk(ctx), llks=m.llks(ds), row_weights=m.row_weights(ds),
                maha=m.mahalanobis(ds)[0], **model_out(new, "it_"), **score_out(m.score_heldout(tr, he), "score_"))


for _d in (40, 300):
    _add("tppca_d%d" % _d, ("ppca_t_em_step", "ppca_t_estep", "ppca_t_heldout_score"), biggest=8 * S.ROBUST_N * _d)(functools.partial(_t_run, _d))


@_add("hppca", ("ppca_h_em_step", "ppca_h_estep", "ppca_h_reconstruct", "ppca_h_heldout_score"), biggest=8 * 130 * 97)
def _hppca(P, ctx):
    x, p, w, (s, c, mu) = S.hetero_case(4)
    ds, prec, m = P.Dataset(x, w, ctx=ctx), P.Dataset(p, ctx=ctx), P.HPPCAModel(s, c, mu, ctx=ctx)
    new, llk = m.iterate_with_llk(ds, prec)
    inf = m.infer(ds, prec)
    tr, he = ds.holdout(0.2, seed=5)
    # (no last_llk: the step keeps its statistics in scratch of its own and leaves the record of the last plain step alone)
    return dict(it_llk=llk, llks=m.llks(ds, prec), states=inf._states, covs=inf._covs,
                smooth=m.smooth(ds, prec).numpy(), extrapolate=m.extrapolate(ds, prec).numpy(), **model_out(new, "it_"),
                **score_out(m.score_heldout(tr, he, prec), "score_"))


# ------------------------------------------------------------------ SparseDataset
@functools.lru_cache(maxsize=None)
def sparse_query(n, d):
    """A query pattern for predict: a few columns per row, some rows without any; (indptr, indices)."""
    rng = np.random.default_rng(600 + n + d)
    q = rng.random((n, d)) < 4.0 / d
    q[::7] = False
    ip = np.concatenate([[0], np.cumsum(q.sum(axis=1))]).astype(np.int64)
    ix = np.nonzero(q)[1].astype(np.int32)
    for a in (ip, ix):
        a.setflags(write=False)
    return ip, ix


def sparse_stats_raw(sp, m):
    L = _L()
    out = np.empty(int(L.lib().ppca_stats_len(m.output_size, max(m.state_size, 1))))
    L.check(L.lib().ppca_sparse_stats_raw(sp._ctx.handle, sp._sh, m._device(sp._ctx).h, L.ptr(out)))
    return out


SPARSE_SYMBOLS = ("ppca_sparse_from_host", "ppca_sparse_em_step", "ppca_sparse_em_accumulate", "ppca_sparse_stats_raw", "ppca_sparse_llk",
                  "ppca_sparse_infer", "ppca_sparse_predict", "ppca_heldout_score_sparse", "ppca_topn_sparse", "ppca_sparse_with_weights",
                  "ppca_sparse_to_host", "ppca_sparse_empty_dimensions")


def _sparse_run(k, P, ctx):
    L = _L()
    n, d = S.SPARSE
    x, w, (s, c, mu) = SC.case(n, d, k)
    sp, m = P.SparseDataset.from_dense(x, w, ctx=ctx, **TILING), P.PPCAModel(s, c, mu, ctx=ctx)
    out = {}
    new, llk = m.iterate_with_llk(sp)
    out.update(model_out(new, "it_"), it_llk=llk, last_llk=last_llk(ctx))
    prior = P.Prior().with_isotropic_noise_prior(2.0, 3.0).with_transformation_precision(0.7)
    out.update(model_out(m.iterate_with_prior(sp, prior), "prior_"))
    out["stats"] = sparse_stats_raw(sp, m)
    acc = DevBuf(P, ctx, out["stats"].size)
    L.check(L.lib().ppca_sparse_em_accumulate(ctx.handle, sp._sh, m._device(ctx).h, acc.ptr))
    out["stats_dev"] = acc.numpy()
    out["llks"], out["llk"] = m.llks(sp), m.llk(sp)
    inf = m.infer(sp)
    out["states"], out["covs"] = inf._states, inf._covs
    out["pred_mean"], out["pred_var"] = m.predict(sp, sparse_query(n, d))
    tr, he = sp.holdout(0.2, seed=5)
    out.update(score_out(m.heldout_score(tr, he), "score_"))
    for kappa in (0.0, 1.0):
        cols, scores = m.recommend(sp, 5, kappa=kappa)
        out.update({"top_cols_%g" % kappa: cols, "top_scores_%g" % kappa: scores})
    flags = (C.c_int32 * d)()
    L.check(L.lib().ppca_sparse_empty_dimensions(sp._sh, flags))
    out["empty"] = list(flags)
    sw = sp.with_weights(2.0 * w)
    wb = np.empty(n)
    L.check(L.lib().ppca_sparse_to_host(sw._sh, None, None, None, L.ptr(wb)))
    out["reweighted_w"], out["reweighted_llk"] = wb, m.llk(sw)
    return out


def _sparse_oracle(k):
    """tests/test_gpu_sparse.py::_check_against_oracle: TOL = 1e-5 under its measures (_rel, _model_errors, the llk against the sum of
    |w llk|)."""
    def check(o, r):
        n, d = S.SPARSE
        x, w, (s, c, mu) = SC.case(n, d, k)

        def rel(got, want):
            return float((np.abs(got - want) / (1.0 + np.abs(want))).max())

        llks = o.llks(x, s, c, mu)
        z, cov = o.infer(x, s, c, mu)
        scale = max(float(np.abs(w * llks).sum()), 1.0)
        assert rel(r["llks"], llks) <= 1e-5 and rel(r["states"], z) <= 1e-5 and rel(r["covs"], cov) <= 1e-5
        want_llk = o.llk(x, s, c, mu, w)
        assert abs(r["llk"] - want_llk) / scale <= 1e-5 and abs(r["it_llk"] - want_llk) / scale <= 1e-5
        s1, c1, m1 = o.iterate(x, s, c, mu, w)
        assert abs(r["it_sigma"] / s1 - 1) <= 1e-5
        assert float(np.abs(r["it_C"] - c1).max() / np.abs(c1).max()) <= 1e-5
        assert float((np.abs(r["it_mean"] - m1) / np.maximum(np.abs(m1), s1)).max()) <= 1e-5
    return check


for _k in SPARSE_KS:
    _add("sparse_ppca_k%d" % _k, SPARSE_SYMBOLS, oracle=_sparse_oracle(_k), biggest=8 * 64 * _k * _k)(functools.partial(_sparse_run, _k))


def _sparse_mix_run(k, P, ctx):
    L = _L()
    n, d = S.SPARSE
    x, w, (sig, cs, ms), lw, _ = SMC.mix_case(n, d, k, 3)
    sp = P.SparseDataset.from_dense(x, w, ctx=ctx, **TILING)
    mix = P.PPCAMix([P.PPCAModel(sig[c], cs[c], ms[c], ctx=ctx) for c in range(3)], lw)
    out = {}
    new, llk = mix.iterate_with_llk(sp)
    out.update(mix_out(new, "it_"), it_llk=llk, last_llk=last_llk(ctx), rows_used=rows_used(ctx, 3))
    out["llks"], out["log_post"] = mix.llks(sp), mix.infer_cluster(sp)
    devs, arr = mix._handles(ctx)
    comp = np.empty((3, n))
    L.check(L.lib().ppca_mix_sparse_component_llks(ctx.handle, sp._sh, arr, 3, L.ptr(comp)))
    out["component_llks"] = comp
    out["pred_mean"], out["pred_var"] = mix.predict(sp, sparse_query(n, d))
    for kappa in (0.0, 1.0):
        cols, scores = mix.recommend(sp, 5, kappa=kappa)
        out.update({"top_cols_%g" % kappa: cols, "top_scores_%g" % kappa: scores})
    return out


def _sparse_fa_run(k, P, ctx):
    n, d = S.SPARSE
    x, w, (noise, c, mu), _ = SFC.fa_case(n, d, k)
    sp, m = P.SparseDataset.from_dense(x, w, ctx=ctx, **TILING), P.FAModel(noise, c, mu, ctx=ctx)
    new, llk = m.iterate_with_llk(sp, min_noise=1e-3)
    pm, pv = m.predict(sp, sparse_query(n, d))
    tr, he = sp.holdout(0.2, seed=5)
    tot, mean, var = sp.column_stats()
    return dict(it_noise=new.noise, it_C=new.transform, it_mean=new.mean, it_llk=llk, last_llk=last_llk(ctx), llks=m.llks(sp), pred_mean=pm,
                pred_var=pv, tot=tot, col_mean=mean, col_var=var, **score_out(m.heldout_score(tr, he), "score_"))


def _sparse_t_run(k, P, ctx):
    n, d = S.SPARSE
    x, w, (s, c, mu) = STC.case(n, d, k)
    sp, m = P.SparseDataset.from_dense(x, w, ctx=ctx, **TILING), P.TPPCAModel(s, c, mu, NU, ctx=ctx, row_compressed=True)
    new, llk = m.iterate_with_llk(sp, estimate_dof=True)
    pm, pv = m.predict(sp, sparse_query(n, d))
    return dict(it_dof=new.dof, it_llk=llk, last_llk=last_llk(ctx), llks=m.llks(sp), row_weights=m.row_weights(sp), maha=m.mahalanobis(sp)[0],
                pred_mean=pm, pred_var=pv, **model_out(new, "it_"))


for _k in SPARSE_KS:
    _add("sparse_mix_k%d" % _k, ("ppca_mix_sparse_em_step", "ppca_mix_sparse_llk", "ppca_mix_sparse_component_llks", "ppca_mix_sparse_predict",
                                 "ppca_mix_topn_sparse", "ppca_mix_last_rows_used"), biggest=8 * 150 * 3)(functools.partial(_sparse_mix_run, _k))
    _add("sparse_fa_k%d" % _k, ("ppca_fa_sparse_em_step", "ppca_scale_columns_sparse", "ppca_sparse_predict", "ppca_heldout_score_sparse"),
         biggest=8 * 64 * _k * _k)(functools.partial(_sparse_fa_run, _k))
    _add("sparse_t_k%d" % _k, ("ppca_t_sparse_em_step", "ppca_t_sparse_estep", "ppca_sparse_predict"), biggest=8 * 150 * _k)(
        functools.partial(_sparse_t_run, _k))


# The five entries of Test B that leave the most behind
POLLUTERS = ("step_guard_256x10", "step_outlier_200x16", "engine_mfma_90x65", "mix_multi_3x4", "sparse_ppca_k16")

# Entries whose bits legitimately depend on something besides their inputs (each with the line that makes it so): none.
BIT_EXEMPT = {e.name: e.exempt_line for e in ENTRIES if e.exempt_line}
