"""MAP priors (prior.rs:8-110; ppca_model.rs:307-308, :360-371, :379-384) in every device M-step kernel.

The transformation precision tau and the inverse-gamma noise prior (alpha, beta) are applied inside the finalisation kernels; the
mean prior is a host solve after them (em_finalize_impl, ppca_capi.hip).  Which kernel finalises a shape (ppca_path_kind):
  fused (d <= 256, k <= 10)   finalize_qprep_kernel<K> (plain step, ppca_em_finalize), finalize_kernel<K> (mixture step component by
                              component), finalize_qprep_multi_kernel<K> (mixture step, all components in one launch)
  generic, k <= 64            gen_rowsolve_kernel + gen_finalize_misc_kernel (67,584 B of dynamic LDS at k = 64)
  generic, k = 65..128        gen_rowsolve_big_kernel + gen_finalize_misc_kernel
The finalisation is first tested on its own, from the oracle's statistics, so that the E-step's fixed-point error stays out and
the tolerances can be tight; then whole steps, mixtures and the composed / sharded forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # north_star tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _row_rel(got, want):
    """Largest over the rows of (the row's max error / the row's own max); an all-zero row must be matched exactly."""
    err = np.abs(got - want).max(axis=1, initial=0.0)
    scale = np.abs(want).max(axis=1, initial=0.0)
    zero = scale == 0.0
    assert np.all(err[zero] == 0.0), np.nonzero(zero & (err != 0.0))
    return float((err[~zero] / scale[~zero]).max(initial=0.0))


def _kernel(d, k):
    """The finalisation kernel a plain step of this shape runs, asserted against ppca_path_kind."""
    from ppca_rs_amd import _lib

    kind = _lib.lib().ppca_path_kind(d, k)
    kk = max(k, 1)  # (state size 0 runs as one zero column)
    if d <= 256 and kk <= 10:
        assert kind == 1, (d, k, kind)
        return f"finalize_qprep_kernel<{kk}>"
    assert kind == 0, (d, k, kind)
    return "gen_rowsolve_kernel" if kk <= 64 else "gen_rowsolve_big_kernel"


def _data(oracle, n, d, k, seed, mask=0.25):
    """Weighted rows with an all-masked row (1), a zero weight (row 2), a fully masked dimension (e0) and a dimension that only the
    zero-weight row observes (e1)."""
    x, _, _ = oracle.synth(n, d, max(k, 1), mask, seed)
    rng = np.random.default_rng(seed + 1)
    x[1] = np.nan
    w = rng.uniform(0.5, 2.0, n)
    w[2] = 0.0
    e0, e1 = d // 3, d // 3 + 1
    x[:, e0] = np.nan
    x[:, e1] = np.nan
    x[2, e1] = 1.5
    c = 0.4 * rng.standard_normal((d, k))
    mu = 0.2 * rng.standard_normal(d)
    return x, w, 0.8, c, mu, (e0, e1)


def _mean_prior(d):
    # tridiagonal (SPD: eigenvalues in [0.3, 0.7]) -- couples the dimensions yet keeps the host's d x d solves cheap at d = 300
    cov = 0.5 * np.eye(d) + 0.1 * (np.eye(d, k=1) + np.eye(d, k=-1))
    return np.linspace(-1.0, 1.0, d), cov


def _priors(P, oracle, d):
    """(name, library prior, oracle prior, tau, has mean prior) for every variant of the hooks."""
    pm, pc = _mean_prior(d)
    out = [("none", None, None, 0.0, False), ("default", P.Prior(), oracle.Prior(), 0.0, False)]
    for tau in (1e-3, 0.7, 1e8):
        out.append((f"tau={tau:g}", P.Prior().with_transformation_precision(tau), oracle.Prior(transformation_precision=tau), tau,
                    False))
    for a, b in ((3.0, 2.0), (0.0, 0.0)):
        out.append((f"ig({a:g},{b:g})", P.Prior().with_isotropic_noise_prior(a, b),
                    oracle.Prior(isotropic_noise_alpha=a, isotropic_noise_beta=b), 0.0, False))
    out.append(("mean", P.Prior().with_mean_prior(pm, pc), oracle.Prior(mean=pm, mean_covariance=pc), 0.0, True))
    out.append(("all", P.Prior().with_mean_prior(pm, pc).with_isotropic_noise_prior(3.0, 2.0).with_transformation_precision(0.7),
                oracle.Prior(mean=pm, mean_covariance=pc, isotropic_noise_alpha=3.0, isotropic_noise_beta=2.0,
                             transformation_precision=0.7), 0.7, True))
    return out


def _download(h, d, k):
    from ppca_rs_amd import _lib

    sig, c, m = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    _lib.check(_lib.lib().ppca_model_download(h, C.byref(sig), _lib.ptr(c), _lib.ptr(m)))
    return sig.value, c, m


def _finalize_dev(ctx, model, stats_dev, prior):
    """ppca_em_finalize of device statistics into a fresh model buffer -> (sigma, C, mean)."""
    from ppca_rs_amd import _lib
    from ppca_rs_amd.api import _prior_ref

    lib = _lib.lib()
    d, k = model.output_size, model.state_size
    out = C.c_void_p()
    _lib.check(lib.ppca_model_alloc(ctx.handle, d, k, C.byref(out)))
    try:
        pref, keep = _prior_ref(prior)
        _lib.check(lib.ppca_em_finalize(ctx.handle, model._device(ctx).h, C.c_void_p(stats_dev.data_ptr()), pref, out))
        return _download(out, d, k)
    finally:
        lib.ppca_model_free(out)


# ------------------------------------------------------------------ 1. the finalisation on its own
FIN_SHAPES = ([(37, k) for k in range(1, 11)] + [(256, k) for k in range(1, 11)] + [(37, 0), (300, 0)]
              + [(200, 11), (200, 13), (200, 16), (300, 17), (300, 33), (300, 63), (300, 64), (150, 65), (152, 96), (149, 128)])


@pytest.mark.parametrize("d,k", FIN_SHAPES, ids=[f"d{d}_k{k}" for d, k in FIN_SHAPES])
def test_finalize_with_each_prior_against_host_and_oracle(P, oracle, d, k):
    """ppca_em_finalize from the oracle's statistics (oracle.stats) with every prior variant, against the host finalisation of the
    same statistics (finalize_host: 1e-10 per row of C, sigma, mean) and the oracle's whole step (oracle.iterate: 1e-9).  The two
    special dimensions keep their old row and mean with tau = 0 and get an exactly-zero row with tau > 0; Prior() is no prior bit for
    bit, IG(0, 0) is not; each hook leaves what it does not touch bit-identical."""
    import torch

    from ppca_rs_amd import _lib
    from ppca_rs_amd.distributed import finalize_host

    _kernel(d, k)
    n = 120
    x, w, s, c, mu, empty = _data(oracle, n, d, k, 40 * d + k)
    ctx = _lib.default_context()
    m = P.PPCAModel(s, c, mu)
    st = oracle.stats(x, s, c if k else np.zeros((d, 1)), mu, w)  # (state size 0: the statistics of one zero column)
    assert st.shape[0] == _lib.lib().ppca_stats_len(d, k)
    for j in empty:
        assert st[oracle.stats_len(d, max(k, 1)) - 8 - d + j] == 0.0  # totals: no weight observes e0 / e1
    dev = torch.from_numpy(st).to("cuda")
    torch.cuda.synchronize()
    got = {}
    for name, pr, opr, tau, has_mean in _priors(P, oracle, d):
        sig, cn, mn = _finalize_dev(ctx, m, dev, pr)
        got[name] = (sig, cn, mn)
        host = finalize_host(m, st, pr)
        assert abs(sig - host.isotropic_noise) <= 1e-10 * host.isotropic_noise, name
        assert _row_rel(cn, host.transform) <= 1e-10, name
        assert _rel(mn, host.mean) <= 1e-10, name
        if k > 0:
            s1, c1, m1 = oracle.iterate(x, s, c, mu, w, opr)
            assert abs(sig - s1) <= 1e-9 * s1, name
            assert _row_rel(cn, c1) <= 1e-9, name
            assert _rel(mn, m1) <= 1e-9, name
        for j in empty:  # ppca_model.rs:313-321 / :373-377
            if tau == 0.0:
                np.testing.assert_array_equal(cn[j], c[j], err_msg=name)
            else:
                np.testing.assert_array_equal(cn[j], np.zeros(k), err_msg=name)
            if not has_mean:
                assert mn[j] == mu[j], name
    none = got["none"]
    for name, (sig, cn, mn) in got.items():
        if name == "default":  # Prior(): no hook set
            assert sig == none[0], name
            np.testing.assert_array_equal(cn, none[1])
            np.testing.assert_array_equal(mn, none[2])
        if name.startswith("tau"):  # tau acts on C only (ppca_model.rs:307-308)
            assert sig == none[0], name
            np.testing.assert_array_equal(mn, none[2], err_msg=name)
            if k > 0:
                assert not np.array_equal(cn, none[1]), name
        if name.startswith("ig"):  # (alpha, beta) act on sigma only (:360-371)
            np.testing.assert_array_equal(cn, none[1], err_msg=name)
            np.testing.assert_array_equal(mn, none[2], err_msg=name)
        if name == "mean":  # the mean prior acts on the mean only (:379-384)
            assert sig == none[0]
            np.testing.assert_array_equal(cn, none[1])
    # IG(0, 0) sets the flag: sigma^2 = (sum / 2) / (N_obs / 2 + 1), not sum / N_obs
    n_obs = float(np.sum(w[:, None] * np.isfinite(x)))
    assert got["ig(0,0)"][0] != none[0]
    assert abs(got["ig(0,0)"][0] ** 2 * (n_obs + 2.0) - none[0] ** 2 * n_obs) <= 1e-12 * none[0] ** 2 * n_obs


# ------------------------------------------------------------------ 2. whole steps
def _block_masked(oracle, n, d, k, seed):
    """One cyclic run of d / 2 masked dimensions per sample (BASELINE config 4)."""
    x, _, _ = oracle.synth(n, d, k, 0.0, seed)
    rng = np.random.default_rng(seed)
    for i in range(n):
        x[i, (rng.integers(0, d) + np.arange(d // 2)) % d] = np.nan
    return x


E2E = [(400, 256, 1, "all"), (400, 255, 1, "all"), (400, 256, 4, "all"), (400, 255, 4, "all"), (400, 256, 10, "all"),
       (400, 255, 10, "all"), (300, 200, 12, "all"), (300, 200, 16, "all"), (300, 300, 20, "all"),
       # (config 4 at oracle-sized N; no mean prior: its host solve is d^3)
       (257, 1024, 64, "tau+ig"), (120, 140, 100, "all"),
       (400, 64, 3, "large-beta"), (400, 200, 5, "small-sigma"), (300, 200, 12, "small-sigma")]


def _e2e_prior(P, oracle, d, which):
    pm, pc = _mean_prior(d)
    if which == "all":
        kw = dict(mean=pm, mean_covariance=pc, isotropic_noise_alpha=3.0, isotropic_noise_beta=2.0, transformation_precision=0.7)
    elif which == "tau+ig":
        kw = dict(isotropic_noise_alpha=3.0, isotropic_noise_beta=2.0, transformation_precision=0.7)
    elif which == "large-beta":  # beta dominates the noise estimate: sigma^2 ~ 1e3 after the first step
        kw = dict(isotropic_noise_alpha=2.0, isotropic_noise_beta=1e7, transformation_precision=0.7)
    else:  # small-sigma: a flat IG(0, 0) and a weak ridge on data with sigma = 1e-2, from near the truth
        kw = dict(isotropic_noise_alpha=0.0, isotropic_noise_beta=0.0, transformation_precision=1e-3)
    pr = P.Prior()
    if "mean" in kw:
        pr = pr.with_mean_prior(kw["mean"], kw["mean_covariance"])
    if "isotropic_noise_alpha" in kw:
        pr = pr.with_isotropic_noise_prior(kw["isotropic_noise_alpha"], kw["isotropic_noise_beta"])
    pr = pr.with_transformation_precision(kw["transformation_precision"])
    return pr, oracle.Prior(**kw)


@pytest.mark.parametrize("n,d,k,which", E2E, ids=[f"d{d}_k{k}_{wh}" for _, d, k, wh in E2E])
def test_em_steps_with_prior_against_oracle(P, oracle, n, d, k, which):
    """PPCAModel.iterate_with_llk(ds, prior), three steps, each against oracle.iterate from the same input model: the model within
    the suite's RTOL (the E-step's fixed-point statistics), the llk of the input model within 1e-9."""
    _kernel(d, k)
    rng = np.random.default_rng(d + 7 * k)
    if d == 1024:
        x = _block_masked(oracle, n, d, k, 700 + d)
    elif which == "small-sigma":
        x, c_true, mu_true = oracle.synth(n, d, k, 0.25, 900 + d, sigma_true=1e-2)
    else:
        x, _, _ = oracle.synth(n, d, k, 0.3, 800 + d + k)
    x[1] = np.nan
    w = rng.uniform(0.5, 1.5, n)
    if which == "small-sigma":
        c, mu, s = c_true + 1e-3 * rng.standard_normal((d, k)), mu_true, 2e-2
    else:
        c, mu, s = 0.3 * rng.standard_normal((d, k)), 0.1 * rng.standard_normal(d), 0.9
    pr, opr = _e2e_prior(P, oracle, d, which)
    ds, m = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    for it in range(3):
        s0, c0, m0 = m.isotropic_noise, m.transform, m.mean
        want_llk = oracle.llk(x, s0, c0, m0, w)
        s1, c1, m1 = oracle.iterate(x, s0, c0, m0, w, opr)
        m, llk = m.iterate_with_llk(ds, pr)
        assert abs(llk - want_llk) < 1e-9 * abs(want_llk), it
        assert abs(m.isotropic_noise - s1) < RTOL * s1, it
        assert _rel(m.transform, c1) < RTOL and _rel(m.mean, m1) < RTOL, it
    if which == "large-beta":
        assert m.isotropic_noise > 10.0


@pytest.mark.parametrize("d,k", [(256, 4), (37, 10), (200, 16)])
def test_huge_precision_shrinks_the_next_pass(P, oracle, d, k):
    """tau = 1e8 shrinks C about 1e8-fold; the next pass runs on that transform -- on the fused path through the slice table that
    finalize_qprep_kernel built from it in the step's own launch.  Its llks against the oracle's at 1e-9, and the second step."""
    _kernel(d, k)
    n = 300
    x, w, s, c, mu, _ = _data(oracle, n, d, k, 77 + d)
    pr = P.Prior().with_transformation_precision(1e8)
    opr = oracle.Prior(transformation_precision=1e8)
    ds = P.Dataset(x, w)
    m1, _ = P.PPCAModel(s, c, mu).iterate_with_llk(ds, pr)
    s1, c1, mu1 = oracle.iterate(x, s, c, mu, w, opr)
    # (S_j is ~1e3 here: against the tau = 0 step the rows shrink ~1e5-fold)
    assert 0.0 < np.abs(m1.transform).max() < 1e-3 * np.abs(P.PPCAModel(s, c, mu).iterate(ds).transform).max()
    assert _rel(m1.transform, c1) < RTOL and abs(m1.isotropic_noise - s1) < RTOL * s1
    want = oracle.llks(x, m1.isotropic_noise, m1.transform, m1.mean)
    assert _rel(m1.llks(ds), want) < 1e-9
    m2, llk = m1.iterate_with_llk(ds, pr)
    want_llk = oracle.llk(x, m1.isotropic_noise, m1.transform, m1.mean, w)
    assert abs(llk - want_llk) < 1e-9 * abs(want_llk)
    s2, c2, mu2 = oracle.iterate(x, m1.isotropic_noise, m1.transform, m1.mean, w, opr)
    assert _rel(m2.transform, c2) < RTOL and abs(m2.isotropic_noise - s2) < RTOL * s2 and _rel(m2.mean, mu2) < RTOL


@pytest.mark.parametrize("d,k", [(256, 10), (200, 16)])
def test_trainer_with_prior_equals_the_manual_loop(P, oracle, d, k):
    """PPCATrainer.train(start=, prior=) is the loop of iterate_with_prior steps, then to_canonical: bit for bit."""
    x, w, s, c, mu, _ = _data(oracle, 500, d, k, 5 + k)
    pr, _ = _e2e_prior(P, oracle, d, "all")
    ds, start = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    got = P.PPCATrainer(ds).train(start=start, prior=pr, state_size=k, n_iters=3, quiet=True)
    loud = P.PPCATrainer(ds).train(start=start, prior=pr, state_size=k, n_iters=3)
    m = start
    for _ in range(3):
        m = m.iterate_with_prior(ds, pr)
    want = m.to_canonical()
    for g in (got, loud):
        assert g.isotropic_noise == want.isotropic_noise
        np.testing.assert_array_equal(g.transform, want.transform)
        np.testing.assert_array_equal(g.mean, want.mean)


# ------------------------------------------------------------------ 3. mixtures
def _mix_data(oracle, n, d, k, nm, seed):
    """nm clusters, weighted rows (positive weights: mix.rs:304-309), an all-masked row; the start near the truth, so that no
    component of so small a dataset collapses onto a few rows."""
    rng = np.random.default_rng(seed)
    parts = [oracle.synth(n // nm, d, k, 0.25, seed + c_, mean_scale=3.0) for c_ in range(nm)]
    x = np.concatenate([p[0] for p in parts])
    x[4] = np.nan
    w = rng.uniform(0.5, 1.5, x.shape[0])
    sig = rng.uniform(0.8, 1.2, nm)
    cs = np.stack([p[1] + 0.3 * rng.standard_normal((d, k)) for p in parts])
    ms = np.stack([p[2] + 0.3 * rng.standard_normal(d) for p in parts])
    lw = np.log(rng.dirichlet(3.0 * np.ones(nm)))
    return x, w, sig, cs, ms, lw


@pytest.mark.parametrize("d,k", [(64, 1), (200, 3), (256, 10)])
def test_mixture_multi_component_finalisation_with_prior(P, oracle, d, k):
    """PPCAMix.iterate_with_llk(ds, prior), weighted, with tau + IG on components of one fused state size: the step finalises every
    component in one launch (finalize_qprep_multi_kernel<K>).  Two steps, each against oracle.mix_iterate from the same input."""
    assert _kernel(d, k).startswith("finalize_qprep_kernel")
    nm = 3
    x, w, sig, cs, ms, lw = _mix_data(oracle, 900, d, k, nm, 60 + k)
    pr = P.Prior().with_isotropic_noise_prior(3.0, 2.0).with_transformation_precision(0.7)
    opr = oracle.Prior(isotropic_noise_alpha=3.0, isotropic_noise_beta=2.0, transformation_precision=0.7)
    ds = P.Dataset(x, w)
    mix = P.PPCAMix([P.PPCAModel(sig[c_], cs[c_], ms[c_]) for c_ in range(nm)], lw)
    plain = mix.iterate(ds)
    for it in range(2):
        sig = np.array([mm.isotropic_noise for mm in mix.models])
        cs, ms, lw = np.stack([mm.transform for mm in mix.models]), np.stack([mm.mean for mm in mix.models]), mix.log_weights
        want = oracle.mix_iterate(x, sig, cs, ms, lw, w, opr)
        want_llk = float(np.dot(w, oracle.mix_llks(x, sig, cs, ms, lw)))
        mix, llk = mix.iterate_with_llk(ds, pr)
        assert abs(llk - want_llk) < 1e-8 * abs(want_llk), it  # (as test_mixture_against_oracle)
        for c_, mdl in enumerate(mix.models):
            assert abs(mdl.isotropic_noise - want[0][c_]) < RTOL * want[0][c_], (it, c_)
            assert _rel(mdl.transform, want[1][c_]) < RTOL and _rel(mdl.mean, want[2][c_]) < RTOL, (it, c_)
        assert _rel(mix.log_weights, want[3]) < RTOL, it
        if it == 0:  # the prior reached the kernel: sigma moves, the mean (old C, same statistics) does not
            for a, b in zip(mix.models, plain.models):
                assert a.isotropic_noise != b.isotropic_noise
                np.testing.assert_array_equal(a.mean, b.mean)


@pytest.mark.parametrize("ks,hooks", [((2, 4, 12), "all"), ((3, 3, 3), "all"), ((3, 3, 3), "mean")])
def test_mixture_component_by_component_with_prior(P, ks, hooks):
    """Mixed state sizes (two fused instantiations and the generic pipeline), or a mean prior on components of one size: the step
    finalises component by component (finalize_kernel<K>, gen_rowsolve_kernel; the mean prior on the host after each).  Two weighted
    steps against the second restatement (oracle/restate_numpy.py, mix.rs:281-337) with the prior (as
    test_mixture_with_different_state_sizes)."""
    from oracle import restate_numpy as R

    rng = np.random.default_rng(29 + sum(ks))
    n, d = 160, 14
    assert [_kernel(d, k) for k in ks] == [f"finalize_qprep_kernel<{k}>" if k <= 10 else "gen_rowsolve_kernel" for k in ks]
    x = rng.standard_normal((n, 3)) @ rng.standard_normal((3, d)) + 0.4 * rng.standard_normal((n, d))
    x[rng.random((n, d)) < 0.25] = np.nan
    x[:, 6] = np.nan  # a fully masked dimension
    w = rng.uniform(0.5, 1.5, n)
    sig = [0.9, 1.1, 0.7]
    cs = [0.6 * rng.standard_normal((d, k)) for k in ks]
    ms = [0.3 * rng.standard_normal(d) for _ in ks]
    lw = np.log(np.array([0.2, 0.5, 0.3]))
    pm, pc = _mean_prior(d)
    pr = P.Prior().with_mean_prior(pm, pc)
    kw = dict(mean=pm, mean_covariance=pc)
    if hooks == "all":
        pr = pr.with_isotropic_noise_prior(3.0, 2.0).with_transformation_precision(0.7)
        kw.update(isotropic_noise_alpha=3.0, isotropic_noise_beta=2.0, transformation_precision=0.7)
    pn = R.PriorN(**kw)
    ds = P.Dataset(x, w)
    mix = P.PPCAMix([P.PPCAModel(s, c, m) for s, c, m in zip(sig, cs, ms)], lw)
    for _ in range(2):
        s1, c1, m1, lw1 = R.mix_iterate(x, np.array(sig), cs, ms, lw, w, pn)
        mix = mix.iterate_with_prior(ds, pr)
        for c_, mdl in enumerate(mix.models):
            assert abs(mdl.isotropic_noise - s1[c_]) < 1e-7 * s1[c_]
            assert _rel(mdl.transform, c1[c_]) < 1e-6 and _rel(mdl.mean, m1[c_]) < 1e-6
            if hooks == "all":
                np.testing.assert_array_equal(mdl.transform[6], np.zeros(mdl.state_size))  # tau > 0: the empty row is 0
        assert _rel(mix.log_weights, lw1) < 1e-8
        sig, cs, ms, lw = list(s1), c1, m1, lw1


# ------------------------------------------------------------------ 4. composed and sharded steps on one GPU
@pytest.mark.parametrize("d,k", [(256, 7), (300, 64), (150, 96)])
def test_composed_and_sharded_steps_with_prior_equal_the_plain_step(P, oracle, d, k):
    """ppca_em_accumulate + ppca_em_finalize(prior), ShardedEM over a single-rank library communicator and ShardedEM over the
    torch stream (no communicator) all equal ppca_em_step(prior) bit for bit, two steps."""
    import torch

    from ppca_rs_amd import _lib
    from ppca_rs_amd.api import _prior_ref
    from ppca_rs_amd.distributed import Communicator, ShardedEM, stats_len

    _kernel(d, k)
    lib = _lib.lib()
    x, w, s, c, mu, _ = _data(oracle, 600, d, k, 3 * d + k)
    pr, _ = _e2e_prior(P, oracle, d, "all" if d <= 256 else "tau+ig")
    ctx = _lib.default_context()
    ds, start = P.Dataset(x, w), P.PPCAModel(s, c, mu)
    want1, llk1 = start.iterate_with_llk(ds, pr)
    want2, llk_second = want1.iterate_with_llk(ds, pr)
    # composed by hand
    stats = torch.zeros(stats_len(d, k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pref, keep = _prior_ref(pr)
    _lib.check(lib.ppca_em_accumulate(ctx.handle, ds._h, start._device(ctx).h, C.c_void_p(stats.data_ptr())))
    out = C.c_void_p()
    _lib.check(lib.ppca_model_alloc(ctx.handle, d, k, C.byref(out)))
    _lib.check(lib.ppca_em_finalize(ctx.handle, start._device(ctx).h, C.c_void_p(stats.data_ptr()), pref, out))
    got = _download(out, d, k)
    lib.ppca_model_free(out)
    ctx.synchronize()
    assert float(stats[-8 + 2].item()) == llk1
    assert got[0] == want1.isotropic_noise
    np.testing.assert_array_equal(got[1], want1.transform)
    np.testing.assert_array_equal(got[2], want1.mean)
    comm = Communicator(ctx, 1, 0, Communicator.unique_id())
    try:
        # (one at a time: a ShardedEM points the context at its own stream until close())
        for make in (lambda: ShardedEM(ds, start, pr, comm=comm), lambda: ShardedEM(ds, start, pr)):
            em = make()
            try:
                for want, want_llk in ((want1, llk1), (want2, llk_second)):
                    em.step()
                    g = em.model()
                    assert em.llk_of_previous() == want_llk
                    assert g.isotropic_noise == want.isotropic_noise
                    np.testing.assert_array_equal(g.transform, want.transform)
                    np.testing.assert_array_equal(g.mean, want.mean)
            finally:
                em.close()
    finally:
        comm.close()


def test_sharded_mixture_with_prior_single_rank_equals_the_plain_step(P, oracle):
    """ShardedMixEM(prior=) over a single-rank library communicator: ppca_mix_em_step_sharded equals PPCAMix.iterate_with_llk with
    the same prior bit for bit -- once with tau + IG (one launch over the components), once with all three hooks (component by
    component)."""
    from ppca_rs_amd import _lib
    from ppca_rs_amd.distributed import Communicator, ShardedMixEM

    ctx = _lib.default_context()
    nm, d, k = 3, 24, 3
    assert _kernel(d, k) == "finalize_qprep_kernel<3>"
    x, w, sig, cs, ms, lw = _mix_data(oracle, 1200, d, k, nm, 91)
    ds = P.Dataset(x, w)
    mix0 = P.PPCAMix([P.PPCAModel(sig[c_], cs[c_], ms[c_]) for c_ in range(nm)], lw)
    pm, pc = _mean_prior(d)
    tau_ig = P.Prior().with_isotropic_noise_prior(3.0, 2.0).with_transformation_precision(0.7)
    comm = Communicator(ctx, 1, 0, Communicator.unique_id())
    try:
        for pr in (tau_ig, tau_ig.with_mean_prior(pm, pc)):
            sm = ShardedMixEM(ds, mix0, pr, comm=comm)
            want = mix0
            for _ in range(2):
                want, want_llk = want.iterate_with_llk(ds, pr)
                assert sm.step() == want_llk
                got = sm.mixture()
                np.testing.assert_array_equal(got.log_weights, want.log_weights)
                for a, b in zip(got.models, want.models):
                    assert a.isotropic_noise == b.isotropic_noise
                    np.testing.assert_array_equal(a.transform, b.transform)
                    np.testing.assert_array_equal(a.mean, b.mean)
    finally:
        comm.close()


# ------------------------------------------------------------------ the dynamic-LDS attribute on a second device
def test_group_step_k64_with_prior_two_devices_when_two_gpus(P, oracle):
    """ppca_em_step_group over two devices at d = 300, k = 64 with tau = 0.7: the second device's finalisation (gen_rowsolve_kernel,
    67,584 B of dynamic LDS) needs hipFuncSetAttribute on THAT device, not only on the first.  Both devices against the
    single-device step.  Skipped on a 1-GPU box."""
    import torch

    from ppca_rs_amd import _lib
    from ppca_rs_amd.api import _prior_ref

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    lib = _lib.lib()
    d, k = 300, 64
    assert _kernel(d, k) == "gen_rowsolve_kernel"
    x, _, _ = oracle.synth(2001, d, k, 0.3, 64)
    rng = np.random.default_rng(64)
    start = P.PPCAModel(0.9, 0.3 * rng.standard_normal((d, k)), np.zeros(d))
    pr = P.Prior().with_transformation_precision(0.7)
    want, want_llk = start.iterate_with_llk(P.Dataset(x), pr)
    ctxs = [_lib.Context(0), _lib.Context(1)]
    half = (len(x) + 1) // 2
    shards = [P.Dataset(x[:half], ctx=ctxs[0]), P.Dataset(x[half:], ctx=ctxs[1])]
    comms = (C.c_void_p * 2)()
    _lib.check(lib.ppca_comm_create_all((C.c_void_p * 2)(ctxs[0].handle, ctxs[1].handle), 2, comms))
    outs = []
    for cx in ctxs:
        h = C.c_void_p()
        _lib.check(lib.ppca_model_alloc(cx.handle, d, k, C.byref(h)))
        outs.append(h)
    start1 = P.PPCAModel(start.isotropic_noise, start.transform, start.mean)  # (a model object caches ONE device copy)
    ins = [start._device(ctxs[0]), start1._device(ctxs[1])]
    pref, keep = _prior_ref(pr)
    llk = C.c_double(0.0)
    try:
        _lib.check(lib.ppca_em_step_group(comms, 2, (C.c_void_p * 2)(shards[0]._h, shards[1]._h), (C.c_void_p * 2)(ins[0].h, ins[1].h),
                                          pref, (C.c_void_p * 2)(*outs), C.byref(llk)))
        assert abs(llk.value - want_llk) < 1e-11 * abs(want_llk)
        got = [_download(h, d, k) for h in outs]
        assert got[0][0] == got[1][0]
        np.testing.assert_array_equal(got[0][1], got[1][1])
        np.testing.assert_array_equal(got[0][2], got[1][2])
        assert abs(got[0][0] - want.isotropic_noise) < 1e-10 * want.isotropic_noise
        assert _rel(got[0][1], want.transform) < 1e-9 and _rel(got[0][2], want.mean) < 1e-9
    finally:
        for h in outs:
            lib.ppca_model_free(h)
        for i in range(2):
            lib.ppca_comm_destroy(comms[i])

