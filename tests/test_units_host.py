"""CPU-only: data in other units (tests/units_cases.py) on everything that runs without a GPU.

  * the premise of tests/test_gpu_units.py, pinned on the fp64 oracle: data, mean and loadings times a = 2^p and the noise level
    times a give bit-identical posteriors and an EM step that is the unscaled one times a, bit for bit; the log-likelihoods follow
    llk - m_i p ln 2 wherever the oracle's own llk stays finite -- and it does NOT stay finite at every scale the library covers (it
    takes the logarithm of a literal LU determinant), which is why the GPU file compares the library with its own unscaled run;
  * the five host finalisers (ppca_em_finalize_host, ppca_fa_finalize_host, ppca_famix_finalize_host, ppca_t_finalize_host,
    ppca_h_finalize_host) on statistics scaled block by block: the new models are bit-identical after un-scaling, for the data's
    units and for the sample weights' (2^q);
  * the numpy restatements the GPU tests of the families lean on;
  * the hold-out split of row-compressed data does not depend on the values.
"""
import numpy as np
import pytest

import units_cases as U

POWERS = (40, -40, 100)
ORACLE_SHAPES = [(97, 33, 3), (130, 200, 10), (70, 256, 16), (60, 300, 20)]


# --------------------------------------------------------------------------- the premise, on the oracle
@pytest.mark.parametrize("n,d,k", ORACLE_SHAPES)
def test_oracle_commutes_with_a_power_of_two(oracle, n, d, k):
    """iterate (weighted and not), infer and reconstruct("smooth") of the fp64 oracle: bit-identical after un-scaling at p = 40, -40
    and 100; llks within the derived bound of llk - m_i p ln 2 on every row whose scaled llk the oracle can still express."""
    cs = U.make_case(n, d, k)
    x, s, c, mu = cs["x"], cs["sigma"], cs["c"], cs["mu"]
    m_i = np.isfinite(x).sum(axis=1)
    base_it = [oracle.iterate(x, s, c, mu, w) for w in (None, cs["w"])]
    base_inf = oracle.infer(x, s, c, mu)
    base_sm = oracle.reconstruct(x, s, c, mu, "smooth")
    base_ll = oracle.llks(x, s, c, mu)
    assert np.isfinite(base_ll).all()
    finite_somewhere = False
    for p in POWERS:
        xs = U.scaled_data(x, p)
        ss, cc, mm = U.scaled_model(s, c, mu, p)
        for w, want in zip((None, cs["w"]), base_it):
            s1, c1, m1 = oracle.iterate(xs, ss, cc, mm, w)
            U.assert_pow2(s1, want[0], p, ("sigma", p))
            U.assert_pow2(c1, want[1], p, ("transform", p))
            U.assert_pow2(m1, want[2], p, ("mean", p))
        st, cv = oracle.infer(xs, ss, cc, mm)
        U.assert_bits(st, base_inf[0], ("states", p))
        U.assert_bits(cv, base_inf[1], ("covariances", p))
        U.assert_pow2(oracle.reconstruct(xs, ss, cc, mm, "smooth"), base_sm, p, ("smooth", p))
        ll = oracle.llks(xs, ss, cc, mm)
        ok = np.isfinite(ll)
        finite_somewhere |= bool(ok.any())
        if ok.any():
            U.assert_llk(ll[ok], base_ll[ok], m_i[ok], p, ("llks", p))
    assert finite_somewhere


def test_oracle_llk_leaves_the_finite_range_at_scale(oracle):
    """Why the oracle is not run on the scaled data by the GPU tests: det(C_o C_o^T + sigma^2 I) of a row, taken literally, is
    a^(2 m): at k = 16, p = 40 it overflows a double on the fully loaded rows."""
    cs = U.make_case(70, 256, 16)
    ss, cc, mm = U.scaled_model(cs["sigma"], cs["c"], cs["mu"], 40)
    ll = oracle.llks(U.scaled_data(cs["x"], 40), ss, cc, mm)
    assert not np.isfinite(ll).all()


# --------------------------------------------------------------------------- the host finalisers
def _em_finalize(hiplib, s, c, mu, stats):
    from ppca_rs_amd import _lib

    d, k = c.shape
    import ctypes as C

    so, co, mo = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    _lib.check(hiplib.ppca_em_finalize_host(d, k, float(s), _lib.ptr(np.ascontiguousarray(c)), _lib.ptr(np.ascontiguousarray(mu)),
                                            _lib.ptr(np.ascontiguousarray(stats)), None, C.byref(so), _lib.ptr(co), _lib.ptr(mo)))
    return so.value, co, mo


def _case_stats(oracle, n, d, k, seed=0):
    cs = U.make_case(n, d, k, seed)
    cs["x"][:, d // 2] = np.nan  # a column with nothing observed keeps its row of the model
    cs["stats"] = oracle.stats(cs["x"], cs["sigma"], cs["c"], cs["mu"], cs["w"])
    xt = np.where(np.isfinite(cs["x"]), cs["x"] - cs["mu"], 0.0)
    cs["sq"] = (cs["w"][:, None] * xt * xt).sum(axis=0)
    return cs


FINAL_SHAPES = [(97, 33, 3), (80, 40, 10), (90, 24, 16), (50, 9, 1)]


@pytest.mark.parametrize("n,d,k", FINAL_SHAPES)
def test_em_finalize_host_in_other_units(hiplib, oracle, n, d, k):
    """(State size 0 reaches the library as one zero column, ppca_model_create: the finaliser itself never sees k = 0.)"""
    cs = _case_stats(oracle, n, d, k)
    s, c, mu, st = cs["sigma"], cs["c"], cs["mu"], cs["stats"]
    base = _em_finalize(hiplib, s, c, mu, st)
    for arr in base:
        U.assert_finite(arr, "base")
    assert base[0] != s  # (the step did something)
    for p in U.POWERS + (100,):
        got = _em_finalize(hiplib, *U.scaled_model(s, c, mu, p), _scaled_keep_llk(st, d, k, p))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))
    for q in U.WEIGHT_POWERS:
        got = _em_finalize(hiplib, s, c, mu, U.scaled_stats(st, d, k, q=q))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_bits(g, b, (name, "weights", q))


def _scaled_keep_llk(st, d, k, p):
    """scaled_stats with the llk scalar (which the finalisers do not read) left as it is instead of NaN."""
    out = U.scaled_stats(st, d, k, p=p)
    a = U.stat_blocks(d, k)[-1][1]
    out[a + 2] = st[a + 2]
    return out


def _fa_finalize(hiplib, psi, c, mu, stats, sq):
    from ppca_rs_amd import _lib

    d, k = c.shape
    po, co, mo = np.empty(d), np.empty((d, k)), np.empty(d)
    _lib.check(hiplib.ppca_fa_finalize_host(d, k, _lib.ptr(np.ascontiguousarray(psi)), _lib.ptr(np.ascontiguousarray(c)),
                                            _lib.ptr(np.ascontiguousarray(mu)), _lib.ptr(np.ascontiguousarray(stats)),
                                            _lib.ptr(np.ascontiguousarray(sq)), None, _lib.ptr(po), _lib.ptr(co), _lib.ptr(mo)))
    return po, co, mo


def _whitened_case(oracle, n, d, k, seed=0):
    """An FA model and the statistics of its whitened form: (psi, c, mu, stats, sq, w)."""
    cs = U.make_case(n, d, k, seed)
    rng = np.random.default_rng(5 + n)
    psi = rng.uniform(0.4, 1.6, d)
    x, c, mu, w = cs["x"], cs["c"], cs["mu"], cs["w"]
    x[:, d // 2] = np.nan
    y, a, mt = x / psi, c / psi[:, None], mu / psi
    stats = oracle.stats(y, 1.0, a, mt, w)
    yt = np.where(np.isfinite(y), y - mt, 0.0)
    return psi, c, mu, stats, (w[:, None] * yt * yt).sum(axis=0), cs


@pytest.mark.parametrize("n,d,k", FINAL_SHAPES)
def test_fa_finalize_host_in_other_units(hiplib, oracle, n, d, k):
    """The whitened statistics are unit-free: the FA model of data times a (one power for all columns, and one power p_j in [-20, 20]
    per column) has noise, transform and mean times a_j, bit for bit -- the division c_j / s_j of a kept row and the products of step 4
    commute with a power of two.  Weights times 2^q scale the statistics and sq and leave the model alone."""
    psi, c, mu, stats, sq, _ = _whitened_case(oracle, n, d, k)
    base = _fa_finalize(hiplib, psi, c, mu, stats, sq)
    for arr in base:
        U.assert_finite(arr, "base")
    pj = np.random.default_rng(9).integers(-20, 21, d)
    for p in (np.array(40), np.array(-40), pj):
        got = _fa_finalize(hiplib, *U.scaled_fa(psi, c, mu, p), stats, sq)
        U.assert_pow2(got[0], base[0], p, ("noise", p))
        U.assert_pow2(got[1], base[1], p[:, None] if p.ndim else p, ("transform", p))
        U.assert_pow2(got[2], base[2], p, ("mean", p))
    for q in U.WEIGHT_POWERS:
        got = _fa_finalize(hiplib, psi, c, mu, U.scaled_stats(stats, d, k, q=q), U.pow2(sq, q))
        for g, b in zip(got, base):
            U.assert_bits(g, b, ("weights", q))


@pytest.mark.parametrize("n,d,k", FINAL_SHAPES[:2])
def test_famix_finalize_host_in_other_units(hiplib, oracle, n, d, k):
    """Three components (their statistics from three differently weighted passes), pooled noise: the same relations."""
    from ppca_rs_amd import _lib

    nm = 3
    psi, c, mu, _, _, cs = _whitened_case(oracle, n, d, k)
    rng = np.random.default_rng(3)
    x, w = cs["x"], cs["w"]
    cc = np.stack([c + 0.1 * rng.standard_normal(c.shape) for _ in range(nm)])
    mm = np.stack([mu + 0.3 * rng.standard_normal(d) for _ in range(nm)])
    resp = rng.dirichlet(np.ones(nm), n).T
    y = x / psi
    stats, sq = [], []
    for q in range(nm):
        mt = mm[q] / psi
        stats.append(oracle.stats(y, 1.0, cc[q] / psi[:, None], mt, w * resp[q]))
        yt = np.where(np.isfinite(y), y - mt, 0.0)
        sq.append(((w * resp[q])[:, None] * yt * yt).sum(axis=0))
    stats, sq = np.ascontiguousarray(np.stack(stats)), np.ascontiguousarray(np.stack(sq))
    scale = np.array([1.0, 0.5, 0.125])

    def fin(psi_, cc_, mm_, stats_, sq_, scale_):
        po, co, mo = np.empty(d), np.empty((nm, d, k)), np.empty((nm, d))
        _lib.check(hiplib.ppca_famix_finalize_host(d, k, nm, _lib.ptr(np.ascontiguousarray(psi_)), _lib.ptr(np.ascontiguousarray(cc_)),
                                                   _lib.ptr(np.ascontiguousarray(mm_)), _lib.ptr(np.ascontiguousarray(stats_)),
                                                   _lib.ptr(np.ascontiguousarray(sq_)), _lib.ptr(scale_), None, _lib.ptr(po), _lib.ptr(co),
                                                   _lib.ptr(mo)))
        return po, co, mo

    base = fin(psi, cc, mm, stats, sq, scale)
    for arr in base:
        U.assert_finite(arr, "base")
    pj = rng.integers(-20, 21, d)
    for p in (np.array(40), np.array(-40), pj):
        got = fin(U.pow2(psi, p), U.pow2(cc, p[:, None] if p.ndim else p), U.pow2(mm, p), stats, sq, scale)
        U.assert_pow2(got[0], base[0], p, ("noise", p))
        U.assert_pow2(got[1], base[1], p[:, None] if p.ndim else p, ("transforms", p))
        U.assert_pow2(got[2], base[2], p, ("means", p))
    for q in U.WEIGHT_POWERS:
        st = np.stack([U.scaled_stats(s_, d, k, q=q) for s_ in stats])
        got = fin(psi, cc, mm, st, U.pow2(sq, q), scale)
        for g, b in zip(got, base):
            U.assert_bits(g, b, ("weights", q))
        got = fin(psi, cc, mm, stats, sq, U.pow2(scale, q))  # (a common factor on the components' scales)
        for g, b in zip(got, base):
            U.assert_bits(g, b, ("scale", q))


def _t_finalize(hiplib, s, c, mu, stats, col):
    import ctypes as C

    from ppca_rs_amd import _lib

    d, k = c.shape
    so, co, mo = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    _lib.check(hiplib.ppca_t_finalize_host(d, k, float(s), _lib.ptr(np.ascontiguousarray(c)), _lib.ptr(np.ascontiguousarray(mu)),
                                           _lib.ptr(np.ascontiguousarray(stats)), _lib.ptr(np.ascontiguousarray(col)), C.byref(so),
                                           _lib.ptr(co), _lib.ptr(mo)))
    return so.value, co, mo


@pytest.mark.parametrize("n,d,k", FINAL_SHAPES)
def test_t_finalize_host_in_other_units(hiplib, oracle, n, d, k):
    """col_sums = V (d x k) | A | T | sq: V and T are unit-free, A scales by a, sq by a^2; all of them by 2^q with the weights."""
    cs = _case_stats(oracle, n, d, k)
    s, c, mu, st = cs["sigma"], cs["c"], cs["mu"], cs["stats"]
    blocks = {name: st[a:b] for name, a, b in U.stat_blocks(d, k)}

    def col(p, q):
        return np.concatenate([U.pow2(blocks["U"], q), U.pow2(blocks["sumx"], p + q), U.pow2(blocks["totals"], q), U.pow2(cs["sq"], 2 * p + q)])

    base = _t_finalize(hiplib, s, c, mu, st, col(0, 0))
    for arr in base:
        U.assert_finite(arr, "base")
    assert base[0] != s
    for p in U.POWERS + (100,):
        got = _t_finalize(hiplib, *U.scaled_model(s, c, mu, p), _scaled_keep_llk(st, d, k, p), col(p, 0))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))
    for q in U.WEIGHT_POWERS:
        got = _t_finalize(hiplib, s, c, mu, U.scaled_stats(st, d, k, q=q), col(0, q))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_bits(g, b, (name, "weights", q))


def _h_finalize(hiplib, s, c, mu, stats):
    import ctypes as C

    from ppca_rs_amd import _lib

    d, k = c.shape
    assert stats.shape[0] == hiplib.ppca_h_stats_len(d, k)
    so, co, mo = C.c_double(0.0), np.empty((d, k)), np.empty(d)
    _lib.check(hiplib.ppca_h_finalize_host(d, k, float(s), _lib.ptr(np.ascontiguousarray(c)), _lib.ptr(np.ascontiguousarray(mu)),
                                           _lib.ptr(np.ascontiguousarray(stats)), C.byref(so), _lib.ptr(co), _lib.ptr(mo)))
    return so.value, co, mo


@pytest.mark.parametrize("n,d,k", FINAL_SHAPES)
def test_h_finalize_host_in_other_units(hiplib, oracle, n, d, k):
    """cross | S | V | A | T | sq | cnt (ppca_h_stats_len).  Two ways to put the data in other units: the noise level times a with the
    precisions as they are (cross, A times a; sq times a^2), and the noise level as it is with the precisions times a_j^-2, one power
    per column (cross, A times a_j^-1; S, V, T times a_j^-2; sq and cnt unit-free): transform and mean times a_j both ways."""
    cs = _case_stats(oracle, n, d, k)
    s, c, mu, st = cs["sigma"], cs["c"], cs["mu"], cs["stats"]
    blocks = {name: st[a:b] for name, a, b in U.stat_blocks(d, k)}
    kp = k * (k + 1) // 2

    def hstats(pc, ps, pa, psq, q=0):
        """powers per column of cross and A (pc), S, V and T (ps), sq (psq)"""
        col = lambda v, width, p: U.pow2(v.reshape(d, width), (np.broadcast_to(p, (d,)) + q)[:, None]).ravel()
        return np.concatenate([col(blocks["cross"], k, pc), col(blocks["S"], kp, ps), col(blocks["U"], k, ps), col(blocks["sumx"], 1, pa),
                               col(blocks["totals"], 1, ps), col(cs["sq"], 1, psq), col(blocks["totals"], 1, 0)])

    zero = np.zeros(d, dtype=np.int64)
    base = _h_finalize(hiplib, s, c, mu, hstats(zero, zero, zero, zero))
    for arr in base:
        U.assert_finite(arr, "base")
    assert base[0] != s
    for p in U.POWERS:
        pv = np.full(d, p)
        got = _h_finalize(hiplib, *U.scaled_model(s, c, mu, p), hstats(pv, zero, pv, 2 * pv))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))
    pj = np.random.default_rng(11).integers(-20, 21, d)
    for pv in (np.full(d, 40), np.full(d, -40), pj):
        got = _h_finalize(hiplib, s, *U.scaled_columns(c, mu, pv), hstats(-pv, -2 * pv, -pv, zero))
        U.assert_bits(got[0], base[0], ("sigma", "precisions"))
        U.assert_pow2(got[1], base[1], pv[:, None], ("transform", "precisions"))
        U.assert_pow2(got[2], base[2], pv, ("mean", "precisions"))
    for q in U.WEIGHT_POWERS:
        got = _h_finalize(hiplib, s, c, mu, hstats(zero, zero, zero, zero, q))
        for g, b, name in zip(got, base, ("sigma", "transform", "mean")):
            U.assert_bits(g, b, (name, "weights", q))


# --------------------------------------------------------------------------- the restatements the GPU tests lean on
def test_fa_restatement_in_other_units():
    """tests/fa_restatement.py (dense numpy, original units): one ECM step of data, noise, loadings and mean times 2^p is the unscaled
    step times 2^p.  The restatement solves with LAPACK, whose pivoting and blocked sums commute with a common power of two."""
    import fa_restatement as R

    cs = U.make_case(60, 9, 3)
    psi = np.random.default_rng(2).uniform(0.4, 1.6, 9)
    base = R.iterate(cs["x"], cs["w"], psi, cs["c"], cs["mu"])
    for p in U.POWERS:
        got = R.iterate(U.scaled_data(cs["x"], p), cs["w"], *U.scaled_fa(psi, cs["c"], cs["mu"], np.array(p)))
        for g, b, name in zip(got, base, ("noise", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))


@pytest.mark.parametrize("dense", [False, True], ids=["kxk", "dense"])
def test_t_restatement_in_other_units(dense):
    """tests/tppca_restatement.py, by the k x k forms and by the m x m covariance: row weights, distances and posterior means bit for
    bit, the ECM step (dof estimated) times a with the same dof, the t log-densities by the llk relation."""
    import tppca_restatement as R

    cs = U.make_case(60, 9, 3)
    x, w, s, c, mu = cs["x"], cs["w"], cs["sigma"], cs["c"], cs["mu"]
    m_i = np.isfinite(x).sum(axis=1)
    base_e, (base_new, base_llk) = R.estep(x, w, s, c, mu, 4.0, dense), R.iterate(x, w, s, c, mu, 4.0, True, dense)
    for p in U.POWERS:
        xs, model = U.scaled_data(x, p), U.scaled_model(s, c, mu, p)
        e, (new, llk) = R.estep(xs, w, *model, 4.0, dense), R.iterate(xs, w, *model, 4.0, True, dense)
        for key in ("u", "delta", "z"):
            U.assert_bits(e[key], base_e[key], (key, p))
        for g, b, name in zip(new[:3], base_new[:3], ("sigma", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))
        U.assert_bits(new[3], base_new[3], ("dof", p))
        U.assert_llk(e["ell"], base_e["ell"], m_i, p, ("ell", p))
        U.assert_llk(llk, base_llk, float(w @ m_i), p, ("llk", p))


def test_known_precision_restatement_in_other_units():
    """tests/hppca_restatement.py (the k x k forms): the noise level times a with the precisions as they are, and the noise level as
    it is with the precisions times a_j^-2 (one power per column) -- posteriors bit for bit, loadings and mean times a_j."""
    import hppca_restatement as R

    cs = U.make_case(60, 9, 3)
    x, w, s, c, mu = cs["x"], cs["w"], cs["sigma"], cs["c"], cs["mu"]
    rng = np.random.default_rng(12)
    prec = np.exp2(rng.uniform(-3.0, 3.0, x.shape))
    obs = np.isfinite(x)
    base_e, (base_new, _) = R.estep(x, prec, w, s, c, mu, False), R.iterate(x, prec, w, s, c, mu, False)
    for p in U.POWERS:
        xs, (ss, cc, mm) = U.scaled_data(x, p), U.scaled_model(s, c, mu, p)
        e, (new, _) = R.estep(xs, prec, w, ss, cc, mm, False), R.iterate(xs, prec, w, ss, cc, mm, False)
        U.assert_bits(e["z"], base_e["z"], ("z", p))
        U.assert_bits(e["Sigma"], base_e["Sigma"], ("Sigma", p))
        for g, b, name in zip(new, base_new, ("sigma", "transform", "mean")):
            U.assert_pow2(g, b, p, (name, p))
        U.assert_llk(e["ell"], base_e["ell"], obs.sum(axis=1), p, ("ell", p))
    pj = rng.integers(-20, 21, x.shape[1])
    xs, (cc, mm), pr = U.scaled_data(x, pj), U.scaled_columns(c, mu, pj), U.scaled_precisions(prec, pj)
    e, (new, _) = R.estep(xs, pr, w, s, cc, mm, False), R.iterate(xs, pr, w, s, cc, mm, False)
    U.assert_bits(e["z"], base_e["z"], "z, columns")
    U.assert_bits(e["Sigma"], base_e["Sigma"], "Sigma, columns")
    U.assert_bits(new[0], base_new[0], "sigma, columns")
    U.assert_pow2(new[1], base_new[1], pj[:, None], "transform, columns")
    U.assert_pow2(new[2], base_new[2], pj, "mean, columns")
    shift, mag = obs @ pj, obs @ np.abs(pj)
    # (sum_O ln p_ij: one logarithm per entry of a scaled argument and their sum, as in FAModel's Jacobian)
    U.assert_llk(e["ell"], base_e["ell"], shift, 1, "ell, columns",
                 U.LLK_ULPS * 2.0 ** -52 * (mag - np.abs(shift)) * U.LN2 + U.log_sum_bound(obs.sum(axis=1), 2 * mag * U.LN2 + 3.0 * U.LN2 * obs.sum(axis=1)))


def test_kmeans_restatement_in_other_units():
    """tests/kmeans_restatement.py: labels and totals identical, sums times a, inertia times a^2."""
    import kmeans_restatement as R

    cs = U.make_case(80, 12, 2)
    rng = np.random.default_rng(4)
    centers = cs["mu"] + rng.standard_normal((3, 12))
    base = R.step(cs["x"], cs["w"], centers, None)
    for p in U.POWERS:
        got = R.step(U.scaled_data(cs["x"], p), cs["w"], U.pow2(centers, p), None)
        for i, (key, power) in enumerate((("labels", 0), ("dist", 2 * p), ("totals", 0), ("sums", p), ("inertia", 2 * p), ("distances", 2 * p))):
            U.assert_pow2(got[i], base[i], power, (key, p)) if i else U.assert_bits(got[i], base[i], key)


# --------------------------------------------------------------------------- the split of row-compressed data
def test_sparse_split_does_not_depend_on_the_values(hiplib):
    """ppca_heldout_split_csr_host sees the pattern alone: the parts of SparseDataset.holdout of data times 2^p hold the same cells,
    with the values times 2^p, and the same counts."""
    import ppca_rs_amd as P

    cs = U.make_case(70, 40, 3)
    base = P.SparseDataset.from_dense(cs["x"], cs["w"]).holdout(0.2, 5)
    assert 0 < base[0].holdout_counts[1] < base[0].holdout_counts[0]
    for p in U.POWERS:
        got = P.SparseDataset.from_dense(U.scaled_data(cs["x"], p), cs["w"]).holdout(0.2, 5)
        assert got[0].holdout_counts == base[0].holdout_counts
        for g, b in zip(got, base):
            (gp, gi, gv), (bp, bi, bv) = g.csr(), b.csr()
            assert np.array_equal(gp, bp) and np.array_equal(gi, bi)
            U.assert_pow2(gv, bv, p, ("values", p))
