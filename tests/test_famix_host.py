"""CPU-only: the surface of the mixture of factor analysers (FAMix, FAMixTrainer, Dataset._column_moments_multi; the three C-ABI entry
points behind them) is exported and declared, ppca_famix_finalize_host -- the M-step on host buffers -- agrees with a dense numpy
restatement in original units (tests/famix_restatement.py), and FAMix's host-side logic (validation, serialisation, canonical form,
whitening) holds."""
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
    for back in (p.FAMix.load(m.dump()), pickle.loads(pickle.dumps(m))):
        assert isinstance(back, p.FAMix)
        assert all(np.array_equal(getattr(back, f), getattr(m, f)) for f in ("noise", "transforms", "means", "log_weights"))
    with pytest.raises(Exception):
        p.FAMix.load(p.FAModel(np.ones(3), np.ones((3, 1)), np.zeros(3)).dump())  # another kind of container
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
