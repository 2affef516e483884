"""The device-side build of SparseDataset on the GPU: SparseDataset.from_device and the device split against
the host constructor and the host split, which are the oracle -- every array and count of the container, through
ppca_index_to_host_sparse, and every consequence (the passes' outputs on a device-born dataset).

Every comparison is an equality of integers or of value bits: the feature computes nothing in floating point, so there is no
tolerance anywhere in this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparse_build_cases as B
import sparse_cases as SC

pytestmark = pytest.mark.gpu

INVALID = -1


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64) if a.dtype == np.float64 else np.ascontiguousarray(a)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _upload(torch, *arrays):
    out = [torch.tensor(np.asarray(a)).cuda() if a is not None else None for a in arrays]
    torch.cuda.synchronize()
    return out


def _dev(P, torch, csr, d, w=None, tiling=(None, None), ctx=None):
    """The device-born dataset of CSR arrays uploaded through torch."""
    t = _upload(torch, csr[0], csr[1], csr[2], w)
    p = [int(x.data_ptr()) if x is not None and x.numel() else 0 for x in t]
    return P.SparseDataset.from_device(p[0], p[1], p[2], len(csr[0]) - 1, d, p[3] or None, ctx=ctx, keepalive=t, block_rows=tiling[0],
                                       segment=tiling[1])


def _host(P, csr, d, w=None, tiling=(None, None), ctx=None):
    return P.SparseDataset(csr[0], csr[1], csr[2], d, w, ctx=ctx, block_rows=tiling[0], segment=tiling[1])


def _index(hiplib, sp):
    """(the container's own fields, the empty-column flags, the blocks in the form of sparse_build_cases.restate) of a dataset's handle."""
    from ppca_rs_amd._lib import check

    h = sp._sh
    nb, core = C.c_int64(-1), np.full(13, -7, dtype=np.int64)
    check(hiplib.ppca_n_blocks_sparse(C.byref(nb), h))
    check(hiplib.ppca_index_to_host_sparse(-1, h, _ptr(core), None, None, None, None, None, None))
    d = int(core[7])
    assert core[8] == nb.value and (core[0], core[1], d) == (len(sp), sp.nnz, sp._d)
    flags = (C.c_int32 * d)()
    check(hiplib.ppca_sparse_empty_dimensions(h, flags))
    blocks = []
    for b in range(nb.value):
        c = np.full(13, -7, dtype=np.int64)
        check(hiplib.ppca_index_to_host_sparse(b, h, _ptr(c), None, None, None, None, None, None))
        counts = dict(zip(B.COUNTS, (int(v) for v in c)))
        cp = np.full(d + 1, -7, dtype=np.int64)
        tr, tv = np.full(counts["nnz"], -7, dtype=np.int32), np.full(counts["nnz"], np.nan)
        rl = np.full(counts["rows"], -7, dtype=np.int32)
        it, lg = np.zeros(counts["n_items"], dtype=B.ITEM), np.zeros(counts["n_long"], dtype=B.LONG)
        check(hiplib.ppca_index_to_host_sparse(b, h, None, _ptr(cp), _ptr(tr), _ptr(tv), _ptr(rl), _ptr(it), _ptr(lg)))
        it2 = np.zeros(counts["n_items"], dtype=B.ITEM)  # (the items alone: the other path through the accessor)
        check(hiplib.ppca_index_to_host_sparse(b, h, None, None, None, None, None, _ptr(it2), None))
        assert it.tobytes() == it2.tobytes()
        blocks.append(dict(counts=counts, col_ptr=cp, t_row=tr, t_val=tv, rowlist=rl, items=it, longs=lg))
    return tuple(int(v) for v in core), np.array(flags[:], dtype=np.int32), blocks


def _index_differs(a, b):
    bad = B.same_index(a[2], b[2])
    if a[0] != b[0]:
        bad.append("core fields %s != %s" % (a[0], b[0]))
    if not np.array_equal(a[1], b[1]):
        bad.append("empty flags")
    return bad


def _csr_same(a, b):
    return all(_same(x, y) for x, y in zip(a.csr(), b.csr())) and _same(a.weights(), b.weights())


CASES = [(name, t, False) for name in B.NAMES for t in B.TILINGS] + [("seams", t, True) for t in B.TILINGS] + [("nnz0", (None, None), True)]


# ------------------------------------------------------------------ 1. the container, array for array
@pytest.mark.parametrize("name,tiling,weighted", CASES, ids=["%s-b%s-s%s-%s" % (n, t[0], t[1], "w" if w else "nw") for n, t, w in CASES])
def test_device_build_equals_host_build(P, hiplib, torch, name, tiling, weighted):
    indptr, indices, values, d = B.case(name)
    w = B.weights_of(name) if weighted else None
    host = _host(P, (indptr, indices, values), d, w, tiling)
    want = _index(hiplib, host)
    dev = _dev(P, torch, (indptr, indices, values), d, w, tiling)
    assert dev._ip is None and dev._ix is None and dev._vals is None  # a handle and no host arrays
    assert (len(dev), dev.nnz, dev.output_size()) == (len(host), host.nnz, host.output_size())
    got = _index(hiplib, dev)
    assert not _index_differs(got, want)
    assert dev._ip is None  # (nothing above fetched the pattern)
    again = _index(hiplib, _dev(P, torch, (indptr, indices, values), d, w, tiling))  # two device builds: the same bytes
    assert not _index_differs(again, got)
    assert _csr_same(dev, host) and dev.empty_dimensions() == host.empty_dimensions()
    assert dev.index_build_seconds() > 0.0
    if name == "seams":  # the third witness
        mine = B.restate(indptr, indices, values, d, *tiling)
        assert not B.same_index(got[2], mine)
        br, seg = B.tiling_of(*tiling)
        assert got[0][2:6] == (br, seg, max(b["counts"]["rows"] for b in mine), max(b["counts"]["n_runs"] for b in mine))
        assert got[0][6] == int((np.diff(indptr) > 0).sum())


@pytest.mark.parametrize("name,tiling", [("seams", B.SEAMS_TILING), ("big", (None, None)), ("wide", (7, 3))])
def test_the_build_and_the_split_do_not_depend_on_the_grid(P, hiplib, torch, name, tiling):
    from ppca_rs_amd import _lib

    indptr, indices, values, d = B.case(name)
    ctx = _lib.Context()
    out = []
    try:
        for limit in (0, 1, 3):
            ctx.set_grid_limit(limit)
            sp = _dev(P, torch, (indptr, indices, values), d, None, tiling, ctx=ctx)
            train, held = sp.holdout(0.3, 5)
            out.append([_index(hiplib, x) for x in (sp, train, held)] + [train.csr(), held.csr()])
    finally:
        ctx.set_grid_limit(0)
    for o in out[1:]:
        for i in range(3):
            assert not _index_differs(o[i], out[0][i])
        assert all(_same(x, y) for i in (3, 4) for x, y in zip(o[i], out[0][i]))


# ------------------------------------------------------------------ 2. consequences: the passes on a device-born dataset
@functools.lru_cache(maxsize=None)
def _conseq_case(which):
    if which == "seams":
        indptr, indices, values, d = B.case("seams")
        k, tiling = 4, B.SEAMS_TILING
    else:
        x, _, _ = SC.case(200, 1500, 16)
        indptr, indices, values = SC.csr_of(x)
        d, k, tiling = 1500, 16, (None, None)
    rng = np.random.default_rng(77)
    n = len(indptr) - 1
    return (indptr, indices, values), d, k, tiling, 0.5 + rng.random(n), (0.6, rng.standard_normal((d, k)), rng.standard_normal(d))


def _outputs(P, sp, k, model):
    s, c, mu = model
    m = P.PPCAModel(s, c, mu)
    out = {"llks": m.llks(sp)}
    inf = m.infer(sp)
    out["states"], out["covs"] = inf.states(), np.stack(inf.covariances())
    new, llk = m.iterate_with_llk(sp)
    out.update(it_sigma=np.float64(new.isotropic_noise), it_C=new.transform, it_mean=new.mean, it_llk=np.float64(llk))
    train, held = sp.holdout(0.2, 3)
    sc = m.heldout_score(train, held)
    out.update(ho_llks=sc.llks, ho_cols=np.stack([sc.columns[q] for q in ("count", "llk", "se", "z2")]), ho_n=np.float64(sc.n_entries))
    cols, scores = m.recommend(sp, 5)
    out.update(rec_cols=cols, rec_scores=scores)
    mix = P.PPCAMix([m, P.PPCAModel(0.8, c[:, ::-1].copy(), mu + 0.1)], [np.log(0.4), np.log(0.6)]).iterate(sp)
    for i, mm in enumerate(mix.models):
        out.update({"mix%d_C" % i: mm.transform, "mix%d_mean" % i: mm.mean, "mix%d_sigma" % i: np.float64(mm.isotropic_noise)})
    out["mix_lw"] = np.asarray(mix.log_weights)
    fa = P.FAModel(np.full(c.shape[0], 0.7), c, mu).iterate(sp)  # (a values view on the core)
    out.update(fa_noise=fa.noise, fa_C=fa.transform, fa_mean=fa.mean)
    return {key: np.asarray(v) for key, v in out.items()}


@pytest.mark.parametrize("which", ["seams", "200x1500"])
def test_every_pass_gives_the_same_bits_on_a_device_born_dataset(P, torch, which):
    csr, d, k, tiling, w, model = _conseq_case(which)
    want = _outputs(P, _host(P, csr, d, w, tiling), k, model)
    got = _outputs(P, _dev(P, torch, csr, d, w, tiling), k, model)
    bad = [key for key in want if not _same(got[key], want[key])]
    assert not bad, bad
    assert np.isfinite(want["it_llk"]) and np.isfinite(want["fa_noise"]).all() and want["rec_cols"].shape == (len(csr[0]) - 1, 5)


# ------------------------------------------------------------------ 3. the split
@functools.lru_cache(maxsize=None)
def _host_seams(weighted=True):
    import ppca_rs_amd as P

    indptr, indices, values, d = B.case("seams")
    return _host(P, (indptr, indices, values), d, B.weights_of("seams") if weighted else None, B.SEAMS_TILING)


@pytest.mark.parametrize("row_offset", [0, 1000, 2 ** 40])
@pytest.mark.parametrize("seed", [0, 17])
def test_device_split_equals_host_split(P, hiplib, torch, seed, row_offset):
    indptr, indices, values, d = B.case("seams")
    host = _host_seams()
    dev = _dev(P, torch, (indptr, indices, values), d, B.weights_of("seams"), B.SEAMS_TILING)
    for f in (0.0, 0.15, 0.5, 1.0):
        want = host.holdout(f, seed, row_offset=row_offset)
        got = dev.holdout(f, seed, row_offset=row_offset)
        forced = host.holdout(f, seed, row_offset=row_offset, on_device=True)  # a host-born dataset uploads first
        for parts in (got, forced):
            for a, b in zip(parts, want):
                assert a._ip is None and a._handle is not None and a.holdout_counts == b.holdout_counts == (want[0].nnz, want[1].nnz)
                assert (len(a), a.nnz) == (len(b), b.nnz)
                assert not _index_differs(_index(hiplib, a), _index(hiplib, b))  # the part's index is the host-built one of the host's part
                assert _csr_same(a, b)
    mid = dev.holdout_range(0.25, 0.6, seed, row_offset=row_offset)
    assert all(_csr_same(a, b) for a, b in zip(mid, host.holdout_range(0.25, 0.6, seed, row_offset=row_offset)))


def test_kfold_holds_every_entry_exactly_once(P, torch):
    indptr, indices, values, d = B.case("seams")
    dev = _dev(P, torch, (indptr, indices, values), d, None, B.SEAMS_TILING)
    folds = dev.kfold(3, 17)
    want = _host_seams(False).kfold(3, 17)
    keys = []
    for (train, held), (wt, wh) in zip(folds, want):
        assert _csr_same(train, wt) and _csr_same(held, wh) and train.nnz + held.nnz == dev.nnz
        ip, ix, _ = held.csr()
        keys.append(np.repeat(np.arange(len(held), dtype=np.int64), np.diff(ip)) * d + ix)
    keys = np.sort(np.concatenate(keys))
    assert np.array_equal(keys, np.repeat(np.arange(len(dev), dtype=np.int64), np.diff(indptr)) * d + indices)


def test_a_values_view_is_split_by_its_own_values(P, hiplib, torch):
    indptr, indices, values, d = B.case("seams")
    dev = _dev(P, torch, (indptr, indices, values), d, None, B.SEAMS_TILING)
    a = 0.25 + np.random.default_rng(3).random(d)
    view, _, _ = dev._scale_columns(a)
    assert view._vals is None
    scaled = view.csr()[2]
    assert not np.array_equal(scaled, values)
    want = _host(P, (indptr, indices, scaled), d, None, B.SEAMS_TILING).holdout(0.4, 9)
    view2, _, _ = dev._scale_columns(a)
    got = view2.holdout(0.4, 9)
    assert view2._vals is None and all(p._ip is None for p in got)  # split on the device, nothing fetched
    for p, q in zip(got, want):
        assert _csr_same(p, q) and not _index_differs(_index(hiplib, p), _index(hiplib, q))


def test_scores_and_selection_on_device_parts(P, torch):
    csr, d, k, tiling, w, (s, c, mu) = _conseq_case("seams")
    host, dev = _host(P, csr, d, w, tiling), _dev(P, torch, csr, d, w, tiling)
    m = P.PPCAModel(s, c, mu)
    a, b = m.heldout_score(*dev.holdout(0.3, 17)), m.heldout_score(*host.holdout(0.3, 17))
    assert _same(a.llks, b.llks) and (a.n_entries, a.n_rows) == (b.n_entries, b.n_rows)
    assert all(_same(a.columns[q], b.columns[q]) for q in ("count", "llk", "se", "z2"))
    got = P.PPCATrainer(dev).select_state_size([2, 3, 4], seed=7, folds=3, n_iters=5)
    want = P.PPCATrainer(host).select_state_size([2, 3, 4], seed=7, folds=3, n_iters=5)
    assert [g[0] for g in got] == [2, 3, 4]
    for g, h in zip(got, want):
        assert np.float64(g[1].mean_llk).tobytes() == np.float64(h[1].mean_llk).tobytes(), (g[0], g[1].mean_llk, h[1].mean_llk)


# ------------------------------------------------------------------ 4. validation
def _plant(kind, indptr, indices, values, d, rows):
    """The arrays with one violation of `kind` planted in each of `rows` (rows of at least two entries)."""
    ip, ix, v = indptr.copy(), indices.copy(), values.copy()
    for r in rows:
        assert ip[r + 1] - ip[r] >= 2
        e = int(ip[r])
        if kind == "monotone":
            ip[r + 1] = ip[r] - 1
        elif kind == "column":
            ix[ip[r + 1] - 1] = d
        elif kind == "negative":
            ix[e] = -1
        elif kind == "equal":
            ix[e + 1] = ix[e]
        elif kind == "decreasing":
            ix[e], ix[e + 1] = ix[e + 1], ix[e]
        elif kind == "nan":
            v[e + 1] = np.nan
        elif kind == "inf":
            v[ip[r + 1] - 1] = -np.inf
    return ip, ix, v


@pytest.mark.parametrize("kind", ["monotone", "column", "negative", "equal", "decreasing", "nan", "inf"])
def test_validation_names_the_lowest_offending_row(P, hiplib, torch, kind):
    from ppca_rs_amd import _lib

    indptr, indices, values, d = B.case("seams")
    n = len(indptr) - 1
    ctx = _lib.Context()
    for rows in ((270, 7), (7, 270), (200, 5)):
        low = min(rows)
        ip, ix, v = _plant(kind, indptr, indices, values, d, rows)
        for limit in (0, 1):
            ctx.set_grid_limit(limit)
            t = _upload(torch, ip, ix, v)
            h = C.c_void_p()
            rc = hiplib.ppca_from_device_sparse(n, d, ctx.handle, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()),
                                                C.c_void_p(t[2].data_ptr()), None, 64, 8, C.byref(h))
            msg = hiplib.ppca_last_error().decode()
            assert rc == INVALID and not h.value and ("row %d" % low) in msg.replace("row_ptr", ""), (rows, msg)
            hh = C.c_void_p()  # the host constructor's words for the same arrays
            assert hiplib.ppca_sparse_from_host(ctx.handle, n, d, _ptr(ip), _ptr(ix), _ptr(v), None, 64, 8, C.byref(hh)) == INVALID
            assert hiplib.ppca_last_error().decode() == msg and not hh.value
    ctx.set_grid_limit(0)
    good = _dev(P, torch, (indptr, indices, values), d, None, B.SEAMS_TILING, ctx=ctx)  # the context is usable afterwards
    assert not _index_differs(_index(hiplib, good), _index(hiplib, _host_seams(False)))


def test_argument_errors_of_the_c_abi(P, hiplib, torch):
    from ppca_rs_amd import _lib

    indptr, indices, values, d = B.case("seams")
    n = len(indptr) - 1
    ctx = _lib.default_context()
    t = _upload(torch, indptr, indices, values)
    p = [C.c_void_p(x.data_ptr()) for x in t]
    h, h2, nb = C.c_void_p(), C.c_void_p(), C.c_int64()
    assert hiplib.ppca_from_device_sparse(n, d, None, p[0], p[1], p[2], None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_from_device_sparse(n, d, ctx.handle, None, p[1], p[2], None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_from_device_sparse(n, d, ctx.handle, p[0], None, p[2], None, 0, 0, C.byref(h)) == INVALID  # nnz > 0, no columns
    assert hiplib.ppca_from_device_sparse(-1, d, ctx.handle, p[0], p[1], p[2], None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_from_device_sparse(n, 0, ctx.handle, p[0], p[1], p[2], None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_from_device_sparse(n, d, ctx.handle, p[0], p[1], p[2], None, -1, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_from_device_sparse(n, d, ctx.handle, p[0], p[1], p[2], None, 0, -1, C.byref(h)) == INVALID
    # one column too few: row 8 has more entries than columns, and lower rows may hold the column that is now out of range -- the words
    # are the host constructor's
    assert hiplib.ppca_from_device_sparse(n, d - 1, ctx.handle, p[0], p[1], p[2], None, 0, 0, C.byref(h)) == INVALID
    msg = hiplib.ppca_last_error().decode()
    assert hiplib.ppca_sparse_from_host(ctx.handle, n, d - 1, _ptr(indptr), _ptr(indices), _ptr(values), None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_last_error().decode() == msg and "row" in msg and not h.value
    lone = _upload(torch, np.array([0, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32), np.ones(3))
    assert hiplib.ppca_from_device_sparse(1, 2, ctx.handle, *[C.c_void_p(x.data_ptr()) for x in lone], None, 0, 0, C.byref(h)) == INVALID
    assert hiplib.ppca_last_error().decode() == "row 0 has more entries than columns" and not h.value
    sp = _host_seams(False)
    for lo, hi, off in ((-0.1, 0.5, 0), (0.6, 0.5, 0), (0.0, 1.5, 0), (float("nan"), 0.5, 0), (0.0, 0.5, -1)):
        assert hiplib.ppca_heldout_split_sparse(lo, hi, 1, off, ctx.handle, sp._sh, C.byref(h), C.byref(h2), None) == INVALID
    assert hiplib.ppca_heldout_split_sparse(0.0, 0.5, 1, 0, ctx.handle, None, C.byref(h), C.byref(h2), None) == INVALID
    assert not h.value and not h2.value
    assert hiplib.ppca_index_to_host_sparse(5, sp._sh, None, None, None, None, None, None, None) == INVALID
    assert hiplib.ppca_index_to_host_sparse(-2, sp._sh, None, None, None, None, None, None, None) == INVALID
    assert hiplib.ppca_n_blocks_sparse(C.byref(nb), None) == INVALID
    assert hiplib.ppca_n_blocks_sparse(C.byref(nb), sp._sh) == 0 and nb.value == 5


# ------------------------------------------------------------------ 5. borrowing
def test_the_input_is_borrowed_and_left_alone(P, hiplib, torch):
    indptr, indices, values, d = B.case("seams")
    w = B.weights_of("seams")
    dev = _dev(P, torch, (indptr, indices, values), d, w, B.SEAMS_TILING)
    t = dev._keepalive
    assert [int(x.data_ptr()) for x in t] and all(x.is_cuda for x in t)
    train, held = dev.holdout(0.3, 5)
    assert train._keepalive is t and held._keepalive is t  # the parts share the borrowed weights
    model = P.PPCAModel(0.6, np.random.default_rng(1).standard_normal((d, 3)), np.zeros(d))
    ll = model.llks(dev)
    sc = model.heldout_score(train, held)
    del dev
    assert _same(train.weights(), w) and np.isfinite(sc.mean_llk) and np.isfinite(ll).all()
    del train, held
    torch.cuda.synchronize()
    for x, a in zip(t, (indptr, indices, values, w)):
        assert _same(x.cpu().numpy(), np.asarray(a))


# ------------------------------------------------------------------ 6. recycled device memory
def _build_and_split(P, hiplib, torch, ctx):
    indptr, indices, values, d = B.case("seams")
    dev = _dev(P, torch, (indptr, indices, values), d, B.weights_of("seams"), B.SEAMS_TILING, ctx=ctx)
    train, held = dev.holdout(0.3, 5)
    view, _, _ = dev._scale_columns(np.full(d, 0.5))
    vt, vh = view.holdout(0.3, 5)
    out = [_index(hiplib, x) for x in (dev, train, held, vt, vh)]
    return out, [x.csr() for x in (train, held, vt, vh)]


def test_dirtied_memory(P, hiplib, torch):
    """The seams case's build and split on a private context: twice as it comes, then after dirty_scratch(0xFF) (every int -1) and
    after (0x3F), all bit for bit equal to a fresh context's."""
    from ppca_rs_amd import _lib

    fresh = _build_and_split(P, hiplib, torch, _lib.Context())
    ctx = _lib.Context()
    try:
        runs = [_build_and_split(P, hiplib, torch, ctx), _build_and_split(P, hiplib, torch, ctx)]
        for fill in (0xFF, 0x3F):
            blocks, nbytes = ctx.dirty_scratch(fill)
            assert blocks >= 1 and nbytes >= 12 * B.case("seams")[1].size, (blocks, nbytes)
            runs.append(_build_and_split(P, hiplib, torch, ctx))
    finally:
        ctx.trim()
    for i, (idx, csrs) in enumerate(runs):
        for got, want in zip(idx, fresh[0]):
            assert not _index_differs(got, want), i
        assert all(_same(x, y) for a, b in zip(csrs, fresh[1]) for x, y in zip(a, b)), i
