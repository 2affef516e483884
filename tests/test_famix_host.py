"""CPU-only: the surface of the mixture of factor analysers (FAMix, FAMixTrainer, Dataset._column_moments_multi; the three C-ABI entry
points behind them) is exported and declared, ppca_famix_finalize_host -- the M-step on host buffers -- agrees with a dense numpy
restatement in original units (tests/famix_restatement.py) and, with one component and no scale, IS ppca_fa_finalize_host byte for
byte; FAMix's host-side logic (validation, serialisation, canonical form, whitening) holds; and the loop that the five trainers share
prints each trainer's line and, when quiet, reads no log-likelihood back."""
import io
import os
import pickle
import re

import numpy as np
import pytest

import fa_restatement as F
import famix_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("ppca_dataset_column_moments_multi", "ppca_famix_finalize_host", "ppca_famix_em_step")


def test_famix_entry_points_exported(hiplib):
    from ppca_rs_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppca_hip.h")).read(), flags=re.S)
    for name in EXPORTS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert hiplib.ppca_abi_version() == 6


def test_famix_python_surface():
    import ppca_rs
    import ppca_rs_amd as p

    for name in ("FAMix", "FAMixTrainer"):
        assert name in p.__all__ and hasattr(ppca_rs, name), name
    assert ppca_rs.FAMix is p.FAMix
    assert callable(getattr(p.Dataset, "_column_moments_multi", None))
    for meth in ("init", "from_ppca_mix", "from_fa", "load", "whitened", "components", "llks", "llk", "infer_cluster", "iterate",
                 "iterate_with_llk", "to_canonical", "sample", "dump", "smooth", "extrapolate"):
        assert callable(getattr(p.FAMix, meth, None)), meth
    for prop in ("noise", "transforms", "means", "log_weights", "weights", "output_size", "state_size", "n_models", "n_parameters"):
        assert isinstance(getattr(p.FAMix, prop, None), property), prop
    assert callable(getattr(p.FAMixTrainer, "train", None))


# --------------------------------------------------------------------------- ppca_famix_finalize_host against the restatement
N, D, K, NM = 400, 9, 3, 3


def _pack(mom):
    """The packed statistics of include/ppca_hip.h (cross [d k] | S [d k'] lower-packed, e = a (a + 1) / 2 + b | U [d k] | sumx [d] |
    totals [d] | scalars [8]) from the moments of one component."""
    cross, S, U, sumx, tot, sq = mom
    k = cross.shape[1]
    lower = [(p, q) for p in range(k) for q in range(p + 1)]
    Sp = np.stack([S[:, p, q] for p, q in lower], axis=1)
    return np.concatenate([cross.ravel(), Sp.ravel(), U.ravel(), sumx, tot, np.zeros(8)])


def _finalize(hiplib, psi, cs, mus, stats, sq, scale, floor):
    from ppca_rs_amd import _lib

    nm, (d, k) = len(cs), cs[0].shape
    assert stats.shape == (nm, hiplib.ppca_stats_len(d, k))
    c_in, m_in = np.ascontiguousarray(np.stack(cs)), np.ascontiguousarray(np.stack(mus))
    stats, sq = np.ascontiguousarray(stats), np.ascontiguousarray(sq)
    po, co, mo = np.empty(d), np.empty((nm, d, k)), np.empty((nm, d))
    _lib.check(hiplib.ppca_famix_finalize_host(d, k, nm, _lib.ptr(psi), _lib.ptr(c_in), _lib.ptr(m_in), _lib.ptr(stats), _lib.ptr(sq),
                                               _lib.ptr(scale), _lib.ptr(floor), _lib.ptr(po), _lib.ptr(co), _lib.ptr(mo)))
    return po, list(co), list(mo)


@pytest.fixture(scope="module")
def case():
    """N = 400, d = 9, k = 3, K = 3; 30 % masked, psi over 15x, weights, an all-masked row, a zero-weight row; column 4 empty everywhere;
    column 6 observed only in rows where component 2 has no responsibility (empty in ONE component); S of (component 1, column 3)
    zeroed (a row that is kept).  The responsibilities are the model's own except for those zeros.  Both sides get the same moments:
    the restatement in original units, the library in whitened units, packed, component c's multiplied by t_c.
    The restatement's batched k x k form (estep / moments: what its `iterate` and `smooth` rest on) is first held against
    fa_restatement's dense m x m density, posterior and row-by-row moments on this data."""
    psi_true = np.geomspace(0.2, 3.0, D)
    x, cs_true, mus_true, _ = R.synth(N, D, K, NM, psi_true, 0.3, 11, separation=0.6)
    x[17] = np.nan
    x[:, 4] = np.nan
    rng = np.random.default_rng(12)
    w = rng.uniform(0.5, 2.0, N)
    w[23] = 0.0
    psi = psi_true * rng.uniform(0.7, 1.4, D)
    cs = [c + 0.2 * psi_true[:, None] * rng.standard_normal((D, K)) for c in cs_true]
    mus = [m + 0.3 * psi_true * rng.standard_normal(D) for m in mus_true]
    logw = R.log_softmax(rng.standard_normal(NM))
    for q in range(NM):
        z, sigma, ll = R.estep(x, psi, cs[q], mus[q])
        dense = F.llks(x, psi, cs[q], mus[q])
        assert np.all(np.abs(ll - dense) <= 1e-11 * (np.abs(dense) + D)) and ll[17] == 0.0
        zr, sr = F.posterior(x[0], psi, cs[q], mus[q])
        assert np.allclose(z[0], zr, rtol=0, atol=1e-12 * max(1.0, np.abs(zr).max())) and np.allclose(sigma[0], sr, rtol=0, atol=1e-13)
        for got, ref in zip(R.moments(x, w, z, sigma, mus[q]), F.moments(x, w, psi, cs[q], mus[q])):
            assert np.all(np.abs(got - ref) <= 1e-11 * max(np.abs(ref).max(), 1e-300))
    resp = np.exp(R.log_posteriors(x, psi, cs, mus, logw))
    resp[np.isfinite(x[:, 6]), 2] = 0.0
    wr = w[:, None] * resp
    moms, white = [], []
    for q in range(NM):
        z, sigma, _ = R.estep(x, psi, cs[q], mus[q])
        moms.append(list(R.moments(x, wr[:, q], z, sigma, mus[q])))
        zw, sw, _ = R.estep(x / psi, np.ones(D), cs[q] / psi[:, None], mus[q] / psi)  # the whitened model on the whitened rows
        white.append(list(R.moments(x / psi, wr[:, q], zw, sw, mus[q] / psi)))
    moms[1][1][3] = 0.0
    white[1][1][3] = 0.0
    t = np.array([3.0, 1.0, 0.04])
    stats = np.stack([t[q] * _pack(white[q]) for q in range(NM)])
    sq = np.stack([t[q] * white[q][5] for q in range(NM)])
    assert white[2][4][6] == 0.0 and white[0][4][6] > 0.0 and all(m[4][4] == 0.0 for m in white)
    return psi, cs, mus, moms, stats, sq, t


def _assert_close(got, want, rel):
    (p1, c1, m1), (p0, c0, m0) = got, want
    assert np.all(np.abs(p1 - p0) <= rel * p0), np.abs(p1 / p0 - 1).max()
    for a, b, ma, mb in zip(c1, c0, m1, m0):
        assert np.abs(a - b).max() <= rel * np.abs(b).max()
        assert np.all(np.abs(ma - mb) <= rel * np.maximum(np.abs(mb), p0))


def test_famix_finalize_host_matches_the_restatement(hiplib, case):
    """fp64 host arithmetic on the same numbers on both sides: 1e-10 relative in psi, every C_c and mean_c."""
    psi, cs, mus, moms, stats, sq, t = case
    free = _finalize(hiplib, psi, cs, mus, stats, sq, 1.0 / t, None)
    _assert_close(free, R.mstep(moms, psi, cs, mus), 1e-10)
    assert np.array_equal(free[1][1][3], cs[1][3]) and free[2][1][3] != mus[1][3]  # the kept row; its mean still moves
    assert free[0][4] == psi[4] and all(np.array_equal(free[1][q][4], cs[q][4]) and free[2][q][4] == mus[q][4] for q in range(NM))
    assert np.array_equal(free[1][2][6], cs[2][6]) and free[2][2][6] == mus[2][6] and free[0][6] != psi[6]  # empty in component 2 only
    moved = np.delete(np.arange(D), [3, 4])  # (column 3: with S_13 = 0 the pooled value may come out <= 0, which keeps psi_3; both sides agree)
    assert np.all(np.abs(free[0][moved] / psi[moved] - 1) > 1e-6)  # (the step did something)
    floor = np.zeros(D)
    floor[2] = 2.0 * free[0][2]
    bound = _finalize(hiplib, psi, cs, mus, stats, sq, 1.0 / t, floor)
    _assert_close(bound, R.mstep(moms, psi, cs, mus, floor), 1e-10)
    assert bound[0][2] == floor[2] and np.array_equal(np.delete(bound[0], 2), np.delete(free[0], 2))


def test_famix_finalize_host_with_one_component_is_the_fa_finalisation(hiplib, case):
    from ppca_rs_amd import _lib

    psi, cs, mus, moms, stats, sq, t = case
    for q in range(NM):
        st, s2 = np.ascontiguousarray(stats[q]), np.ascontiguousarray(sq[q])
        po, co, mo = np.empty(D), np.empty((D, K)), np.empty(D)
        _lib.check(hiplib.ppca_fa_finalize_host(D, K, _lib.ptr(psi), _lib.ptr(np.ascontiguousarray(cs[q])), _lib.ptr(mus[q]), _lib.ptr(st),
                                                _lib.ptr(s2), None, _lib.ptr(po), _lib.ptr(co), _lib.ptr(mo)))
        for scale in (None, np.ones(1)):
            _assert_close(_finalize(hiplib, psi, [cs[q]], [mus[q]], st[None], s2[None], scale, None), (po, [co], [mo]), 1e-13)


@pytest.mark.parametrize("d,k", [(1, 1), (5, 0), (7, 3), (33, 10), (64, 16)])
def test_fa_finalize_host_is_famix_finalize_host_with_one_component_byte_for_byte(hiplib, d, k):
    """ppca_fa_finalize_host against ppca_famix_finalize_host(n_comp = 1, scale = NULL) on the same buffers: noise, transform and mean
    agree in every byte.  Random SPD S_j; where d > 2 column 1 is unobserved (all of its statistics zero) and S of column 2 is negated (the
    old row is kept); with and without a noise floor; with the sq the statistics imply and with sq = 0, where the variance comes out
    negative and the noise must stay as it was (or at its floor)."""
    from ppca_rs_amd import _lib

    rng = np.random.default_rng(100 * d + k)
    ki = max(k, 1)  # (state size 0: the statistics of one zero column)
    psi, c, mu = rng.uniform(0.2, 3.0, d), np.ascontiguousarray(rng.standard_normal((d, k))), rng.standard_normal(d)
    g = rng.standard_normal((d, ki, ki + 2))
    tot = rng.uniform(50.0, 90.0, d)
    mom = [rng.standard_normal((d, ki)), tot[:, None, None] * (g @ g.transpose(0, 2, 1)) / (ki + 2), rng.standard_normal((d, ki)),
           tot * rng.uniform(-1.0, 1.0, d), tot, None]  # (|delta| <= 1: the variance under sq_fit stays positive)
    if d > 2:
        for a in mom[:4]:
            a[1] = 0.0
        tot[1] = 0.0
        mom[1][2] = -mom[1][2]
    stats = _pack(mom)
    assert stats.shape == (hiplib.ppca_stats_len(d, k),)
    sq_fit = tot * rng.uniform(2.0, 5.0, d) + 4.0 * np.abs(mom[0]).sum(axis=1)
    for sq in (sq_fit, np.zeros(d)):
        for floor in (None, rng.uniform(0.1, 2.5, d)):
            fa = np.empty(d), np.empty((d, k)), np.empty(d)
            mix = np.empty(d), np.empty((1, d, k)), np.empty((1, d))
            _lib.check(hiplib.ppca_fa_finalize_host(d, k, _lib.ptr(psi), _lib.ptr(c), _lib.ptr(mu), _lib.ptr(stats), _lib.ptr(sq),
                                                    _lib.ptr(floor), *(_lib.ptr(o) for o in fa)))
            _lib.check(hiplib.ppca_famix_finalize_host(d, k, 1, _lib.ptr(psi), _lib.ptr(c), _lib.ptr(mu), _lib.ptr(stats), _lib.ptr(sq), None,
                                                       _lib.ptr(floor), *(_lib.ptr(o) for o in mix)))
            for got, want in zip(fa, mix):
                assert got.tobytes() == want.tobytes()
            if d > 2:
                assert np.array_equal(fa[1][2], c[2]) and np.array_equal(fa[1][1], c[1]) and fa[2][1] == mu[1]  # kept rows, unmoved mean
                assert fa[0][1] == max(psi[1], 0.0 if floor is None else floor[1])
            if sq is not sq_fit:
                assert np.array_equal(fa[0], psi if floor is None else np.maximum(psi, floor))
            elif floor is None:  # (the step did something; column 2, its S negated, may keep its noise)
                moved = np.flatnonzero(tot > 0.0)
                assert np.all(fa[0][moved[moved != 2]] != psi[moved[moved != 2]])


def test_famix_finalize_host_scale_undoes_a_factor_on_a_component(hiplib, case):
    """Component c's statistics and sq multiplied by t with scale_c = 1 / t: the result does not move (1e-12)."""
    psi, cs, mus, moms, stats, sq, t = case
    base = _finalize(hiplib, psi, cs, mus, stats / t[:, None], sq / t[:, None], None, None)
    _assert_close(_finalize(hiplib, psi, cs, mus, stats, sq, 1.0 / t, None), base, 1e-12)
    u = np.array([1e-30, 7.0, 1e25])
    _assert_close(_finalize(hiplib, psi, cs, mus, stats * u[:, None], sq * u[:, None], 1.0 / (t * u), None), base, 1e-12)


def test_famix_finalize_host_rejects_bad_arguments(hiplib, case):
    from ppca_rs_amd import PPCAError

    psi, cs, mus, moms, stats, sq, t = case
    bad = psi.copy()
    bad[0] = 0.0
    with pytest.raises(PPCAError):
        _finalize(hiplib, bad, cs, mus, stats, sq, None, None)
    with pytest.raises(PPCAError):
        _finalize(hiplib, psi, cs, mus, stats, sq, np.array([1.0, -1.0, 1.0]), None)
    with pytest.raises(PPCAError):
        _finalize(hiplib, psi, cs, mus, stats, sq, np.array([1.0, np.nan, 1.0]), None)


# --------------------------------------------------------------------------- FAMix host logic
def _mix(d=6, k=2, nm=3, seed=3):
    import ppca_rs_amd as p

    rng = np.random.default_rng(seed)
    return p.FAMix(rng.uniform(0.1, 4.0, d), rng.standard_normal((nm, d, k)), rng.standard_normal((nm, d)), rng.standard_normal(nm))


def test_famix_constructor_errors_and_getters():
    import ppca_rs_amd as p

    c, mu, lw = np.ones((2, 4, 3)), np.zeros((2, 4)), np.zeros(2)
    with pytest.raises(ValueError):
        p.FAMix(np.ones(3), c, mu, lw)  # noise of the wrong length
    with pytest.raises(ValueError):
        p.FAMix(1.0, c, mu, lw)  # one level per column, not a scalar
    for bad in (0.0, -1.0, np.nan, np.inf):
        n = np.ones(4)
        n[2] = bad
        with pytest.raises(ValueError):
            p.FAMix(n, c, mu, lw)
    with pytest.raises(TypeError):
        p.FAMix(np.ones(4), np.ones((4, 3)), mu, lw)  # transforms must be (K, d, k)
    with pytest.raises(TypeError):
        p.FAMix(np.ones(4), c, np.zeros(4), lw)  # means must be (K, d)
    with pytest.raises(ValueError):
        p.FAMix(np.ones(4), c, np.zeros((3, 4)), lw)
    with pytest.raises(ValueError):
        p.FAMix(np.ones(4), c, np.zeros((2, 5)), lw)
    with pytest.raises(ValueError):
        p.FAMix(np.ones(4), c, mu, np.zeros(3))
    m = p.FAMix(np.ones(4), c, mu, np.log([1.0, 3.0]))
    assert (m.output_size, m.state_size, m.n_models, m.n_parameters) == (4, 3, 2, 4 + 2 * (4 * 3 + 4) + 1)
    assert np.allclose(m.weights, [0.25, 0.75], rtol=1e-15) and abs(np.exp(m.log_weights).sum() - 1) < 1e-15  # normalised
    got = m.noise
    got[0] = 7.0
    assert m.noise[0] == 1.0  # the getters hand out copies


def test_famix_dump_load_and_pickle_round_trip():
    import ppca_rs_amd as p

    m = _mix()
    m = p.FAMix(m.noise, m.transforms, np.where(m.means > 1.0, -0.0, m.means), m.log_weights)  # (a sign bit that == does not see)
    fields = ("noise", "transforms", "means", "log_weights")
    for back in (p.FAMix.load(m.dump()), pickle.loads(pickle.dumps(m))):
        assert isinstance(back, p.FAMix)
        assert all(getattr(back, f).tobytes() == getattr(m, f).tobytes() and getattr(back, f).shape == getattr(m, f).shape for f in fields)
    z = np.load(io.BytesIO(m.dump()), allow_pickle=False)
    assert z.files == ["kind"] + list(fields) and str(z["kind"]) == "ppca_rs_amd.FAMix"
    assert all(z[f].dtype == np.float64 and z[f].tobytes() == getattr(m, f).tobytes() for f in fields)
    with pytest.raises(Exception) as err:
        p.FAMix.load(p.FAModel(np.ones(3), np.ones((3, 1)), np.zeros(3)).dump())  # another kind of container
    assert type(err.value) is Exception and str(err.value) == "not an FAMix container: ppca_rs_amd.FAModel"
    with pytest.raises(Exception):
        p.FAMix.load(b"not a container")


def test_famix_whitened_components_and_canonical_form_keep_the_shapes():
    import ppca_rs_amd as p

    m = _mix(d=7, k=3, nm=2)
    wh = m.whitened()
    assert isinstance(wh, p.PPCAMix) and np.array_equal(wh.log_weights, m.log_weights)
    for q, (pm, fm) in enumerate(zip(wh.models, m.components())):
        assert pm.isotropic_noise == 1.0 and isinstance(fm, p.FAModel)
        assert np.array_equal(pm.transform, m.transforms[q] / m.noise[:, None]) and np.array_equal(pm.mean, m.means[q] / m.noise)
        assert np.array_equal(fm.noise, m.noise) and np.array_equal(fm.transform, m.transforms[q]) and np.array_equal(fm.mean, m.means[q])
    c = m.to_canonical()
    assert c.n_parameters == m.n_parameters and c.transforms.shape == m.transforms.shape and c.means.shape == m.means.shape
    assert np.array_equal(c.noise, m.noise) and np.array_equal(c.means, m.means) and np.array_equal(c.log_weights, m.log_weights)
    for q in range(2):
        assert np.array_equal(c.transforms[q], p.PPCAModel(1.0, m.transforms[q], m.means[q]).to_canonical().transform)
        assert np.allclose(c.transforms[q] @ c.transforms[q].T, m.transforms[q] @ m.transforms[q].T, rtol=0, atol=1e-12 * np.abs(m.transforms).max() ** 2)
    back = p.FAMix.from_fa(m.components(), m.log_weights)
    assert np.array_equal(back.transforms, m.transforms) and np.array_equal(back.noise, m.noise) and np.array_equal(back.log_weights, m.log_weights)
    other = p.FAModel(m.noise * 2.0, m.transforms[1], m.means[1])
    with pytest.raises(ValueError):
        p.FAMix.from_fa([m.components()[0], other], np.zeros(2))  # the noise is shared
    iso = p.PPCAMix([p.PPCAModel(0.5, m.transforms[0], m.means[0]), p.PPCAModel(0.5, m.transforms[1], m.means[1])], [0.0, 1.0])
    fm = p.FAMix.from_ppca_mix(iso)
    assert np.array_equal(fm.noise, np.full(7, 0.5)) and np.array_equal(fm.transforms, m.transforms) and np.array_equal(fm.log_weights, iso.log_weights)
    with pytest.raises(ValueError):
        p.FAMix.from_ppca_mix(p.PPCAMix([p.PPCAModel(0.5, m.transforms[0], m.means[0]), p.PPCAModel(0.6, m.transforms[1], m.means[1])], [0.0, 0.0]))


# --------------------------------------------------------------------------- the loop of the five trainers
class _StubDataset:
    def __len__(self):
        return 10

    def column_stats(self):
        return None, None, np.array([4.0, 9.0])


class _StubModel:
    """Records what a trainer calls; the llk of generation g is -50 (g + 1)."""
    n_parameters = 7
    _estimated = False

    def __init__(self, calls, gen=0):
        self.calls, self.gen = calls, gen

    def _next(self, name, args):
        self.calls.append((name,) + args)
        return _StubModel(self.calls, self.gen + 1)

    def iterate(self, dataset, *args):
        return self._next("iterate", args)

    def iterate_with_prior(self, dataset, *args):
        return self._next("iterate_with_prior", args)

    def iterate_with_llk(self, dataset, *args):
        return self._next("iterate_with_llk", args), -50.0 * (self.gen + 1)

    def to_canonical(self):
        self.calls.append(("to_canonical",))
        return self


TRAINERS = [("PPCATrainer", "PPCA", dict(state_size=2)), ("PPCAMixTrainer", "PPCA mix", dict(n_models=2, state_size=2)),
            ("FATrainer", "FA", dict(state_size=2)), ("FAMixTrainer", "FA mix", dict(n_models=2, state_size=2)),
            ("TPPCATrainer", "t-PPCA", dict(state_size=2, estimate_dof=True))]


@pytest.mark.parametrize("name,label,kwargs", TRAINERS)
def test_trainer_prints_its_line_and_quiet_reads_no_llk(capsys, name, label, kwargs):
    """Each trainer over a stub model and dataset (n = 10, 7 parameters, llk -50 then -100): the exact printed lines for every metric,
    the extra argument each hands to its model's step (the prior; the floor ratio x the columns' standard deviation; estimate_dof), the
    parameter TPPCATrainer counts for a dof that is about to be estimated, and with quiet=True `iterate` alone (`iterate_with_prior`
    alone for the PPCA trainers given a prior), nothing printed."""
    import ppca_rs_amd as p

    trainer = getattr(p, name)(_StubDataset())
    n_par = 8 if name == "TPPCATrainer" else 7
    fa, ppca = name in ("FATrainer", "FAMixTrainer"), name in ("PPCATrainer", "PPCAMixTrainer")
    extra = (None,) if ppca else (True,) if name == "TPPCATrainer" else None
    want = {"llk": [-50.0 / 10, -100.0 / 10], "aic": [2.0 * (n_par + 50.0) / 10, 2.0 * (n_par + 100.0) / 10],
            "bic": [(-50.0 - n_par * np.log(10)) / 10, (-100.0 - n_par * np.log(10)) / 10]}
    assert want["llk"] == [-5.0, -10.0]
    for metric in ("llk", "aic", "bic"):
        calls = []
        out = trainer.train(start=_StubModel(calls), n_iters=2, metric=metric, **kwargs)
        assert out.gen == 2 and [c[0] for c in calls] == ["iterate_with_llk", "iterate_with_llk", "to_canonical"]
        assert capsys.readouterr().out == "".join(f"Masked {label} iteration {i + 1}: {metric}={want[metric][i]}\n" for i in range(2))
        if fa:
            assert all(len(c) == 2 and np.array_equal(c[1], 1e-3 * np.array([2.0, 3.0])) for c in calls[:2])
        else:
            assert calls[:2] == [("iterate_with_llk",) + extra] * 2
    assert capsys.readouterr().out == ""
    calls = []
    out = trainer.train(start=_StubModel(calls), n_iters=3, quiet=True, **kwargs)
    assert out.gen == 3 and [c[0] for c in calls] == ["iterate"] * 3 + ["to_canonical"] and capsys.readouterr().out == ""
    if fa:
        assert all(np.array_equal(c[1], 1e-3 * np.array([2.0, 3.0])) for c in calls[:3])
    else:
        assert calls[:3] == [("iterate",) + (() if ppca else extra)] * 3
    if ppca:
        calls, prior = [], object()
        trainer.train(start=_StubModel(calls), prior=prior, n_iters=2, quiet=True, **kwargs)
        assert calls == [("iterate_with_prior", prior)] * 2 + [("to_canonical",)] and capsys.readouterr().out == ""
        calls = []
        trainer.train(start=_StubModel(calls), prior=prior, n_iters=1, **kwargs)
        assert calls == [("iterate_with_llk", prior), ("to_canonical",)]
        assert capsys.readouterr().out == f"Masked {label} iteration 1: aic={2.0 * (7 + 50.0) / 10}\n"
    if name == "TPPCATrainer":  # a dof that is not estimated, or was estimated before: no extra parameter
        trainer.train(start=_StubModel([]), n_iters=1, state_size=2)
        assert capsys.readouterr().out == f"Masked t-PPCA iteration 1: aic={2.0 * (7 + 50.0) / 10}\n"
        again = _StubModel([])
        again._estimated = True
        trainer.train(start=again, n_iters=1, **kwargs)
        assert capsys.readouterr().out == f"Masked t-PPCA iteration 1: aic={2.0 * (7 + 50.0) / 10}\n"
