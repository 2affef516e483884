"""Times the output passes that share the per-sample core with the EM pass (llk, llks, infer, smooth,
extrapolate, covariance diagonal, posterior sample / impute, leave-one-out predictive) through the public API, device-resident inputs (diagnostic);
then the host posterior sampler (infer + numpy) on a slice of at most 1 M rows.  `--mix NM` adds the mixture's leave-one-out
predictive over NM components next to its extrapolated covariance diagonal.  `--fa` runs ONLY the legs of the factor-analysis
pass: the column-scale pass with and without output against a device-to-device hipMemcpy of the same N x d array
in the same process, and one FA iteration against one PPCA iteration; every repetition timed on its own (median, min, max).
`--famix NM` runs ONLY the legs of the FA mixture, in one process: the sums-only scale pass, the multi-component
column sweep at NM components (device-resident weights), ppca_mix_em_step and ppca_famix_em_step at NM components, and the parts the
difference of the two goes to (the whitening pass, the sweep, the host finalisation).  `--moments` runs ONLY the legs of the
pairwise second moments, in one process: the pass without and with `cross`, one PPCA iteration (ppca_em_step at
state size k) and the device-to-device copy of X; per pass the multiple of one EM iteration and the fraction of the measured fp64
MFMA rate (profiles/r04/mfma_peak.txt), counting n d (d + 1) flop per symmetric matrix.  `--kmeans K` runs ONLY the legs of masked
k-means and the k-means start, in one process: the fused Lloyd step, the labelling-only call, the two-sweep composition
the fused step replaces (a labelling call, then ppca_dataset_column_moments_multi with one-hot weights), the sums-only scale pass (one
read of X: the floor), the whole `Dataset.kmeans` (seeding plus iterations), the K moment passes of `from_kmeans`, and one
ppca_mix_em_step at K components.  `--robust` runs ONLY the legs of Student-t PPCA, in one process: the sweep with and
without the scaled rows, a whole TPPCAModel.iterate, and the passes they are compared with (PPCAModel.llks, the column-scale pass,
PPCAModel.iterate).  `--hetero` runs ONLY the legs of PPCA with a precision per entry, in one process, alternating:
the sweep alone (HPPCAModel.llks), a whole HPPCAModel.iterate, PPCAModel.llks and PPCAModel.iterate on the same rows, and the
device-to-device copy of X whose rate prices the traffic floor of the iteration (X and P read twice, the records written and read
once).  `--heldout` runs ONLY the legs of held-out scoring, in one process, alternating: the device split, the
score, PPCAModel.loo_llks and the scale pass with output for comparison, and the composition the feature replaces (extrapolate, the
extrapolated covariance diagonal and both downloads).  `--sparse DENSITY` / `--sparse-rows M [--k2 K2]` run ONLY the legs of
SparseDataset (see sparse_legs); with `--sparse-heldout` beside either, ONLY the legs of held-out scoring on that
data (see sparse_heldout_legs); with `--sparse-topn N_TOP` beside either, ONLY the legs of PPCAModel.recommend on that
data (see sparse_topn_legs); with `--mix NM` beside either, ONLY the legs of PPCAMix on that data (see
sparse_mix_legs); with `--sparse-topn N_TOP` and `--mix NM` together, ONLY the legs of PPCAMix.recommend (see
sparse_mix_topn_legs); with `--fa` beside either, ONLY the legs of FAModel on that data (see sparse_fa_legs); with
`--robust` beside either, ONLY the legs of TPPCAModel on that data (see sparse_t_legs); with `--sparse-h` beside
either, ONLY the legs of HPPCAModel on that data (see sparse_h_legs); with `--sparse-build` beside either, ONLY the
legs of the device-side build and split against the host's (see sparse_build_legs)."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppca_rs_amd as P
from ppca_rs_amd import _lib

n, d, k = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
ctx = _lib.default_context()


def sparse_data():
    """The data of the SparseDataset legs, made on the device: (torch, device, rows_mode, rows, cols, vals, mask, indptr, nnz).
    `--sparse DENSITY`: every entry of N x d exists with that probability (mask: the N x d pattern); `--sparse-rows M`: row lengths
    log-normal with mean M (long-tailed), columns uniform (mask: None).  Values from a true model of state size K with noise 0.5."""
    import torch

    dev = "cuda"
    torch.manual_seed(11)
    rows_mode = "--sparse-rows" in sys.argv
    mask = None
    kt = k
    ct = torch.randn((d, kt), dtype=torch.float64, device=dev)
    mt = torch.randn(d, dtype=torch.float64, device=dev)
    if rows_mode:
        per = float(sys.argv[sys.argv.index("--sparse-rows") + 1])
        lengths = torch.exp(torch.randn(n, device=dev) + (np.log(per) - 0.5)).floor().clamp(1, d).long()
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lengths)
        key = torch.unique(rows * d + torch.randint(0, d, (rows.numel(),), device=dev), sorted=True)  # sorted by (row, column), no duplicates
        rows, cols = key // d, key % d
        del key
        counts = torch.bincount(rows, minlength=n)
    else:
        density = float(sys.argv[sys.argv.index("--sparse") + 1])
        mask = torch.rand((n, d), device=dev) < density
        nz = mask.nonzero()
        rows, cols = nz[:, 0].contiguous(), nz[:, 1].contiguous()
        del nz
        counts = mask.sum(dim=1)
    zt = torch.randn((n, kt), dtype=torch.float64, device=dev)
    vals = torch.empty(rows.numel(), dtype=torch.float64, device=dev)
    step = 1 << 25
    for a in range(0, rows.numel(), step):
        r, c = rows[a:a + step], cols[a:a + step]
        vals[a:a + step] = (ct[c] * zt[r]).sum(dim=1) + mt[c] + 0.5 * torch.randn(r.numel(), dtype=torch.float64, device=dev)
    indptr = np.concatenate([[0], np.cumsum(counts.cpu().numpy())]).astype(np.int64)
    nnz = int(rows.numel())
    lens = np.diff(indptr)
    print(f"SparseDataset legs: N = {n}, d = {d}, nnz = {nnz} ({nnz / n / d:.4%} of N x d; {nnz / n:.1f} per row, median {np.median(lens):.0f}, "
          f"max {lens.max()}); dense form {8.0 * n * d / 1e9:.1f} GB", flush=True)
    del zt
    return torch, dev, rows_mode, rows, cols, vals, mask, indptr, nnz


def sparse_legs(reps=5):
    """SparseDataset, in one process, alternating, every repetition timed on its own.  `--sparse DENSITY`: every entry
    of N x d exists with that probability; the sparse llks / iterate next to PPCAModel.llks / iterate on the same data as a dense
    Dataset and the device-to-device copy of that array.  `--sparse-rows M`: a shape the dense layout cannot hold -- row lengths
    log-normal with mean M (long-tailed), columns uniform; the sparse legs alone, at state size K and (with `--k2 K2`) K2, and the host
    time of the index build.  The data is made on the device (before the dense dataset of the other legs, which this leg never
    builds).  Floor: per entry 12 B of CSR, 8 k B of C, 12 B of index and 8 (k + k' + 1) B of record gathered; per row the record
    written once; priced at the copy's rate."""
    torch, dev, rows_mode, rows, cols, vals, mask, indptr, nnz = sparse_data()
    t0 = time.perf_counter()
    sp = P.SparseDataset(indptr, cols.int().cpu().numpy(), vals.cpu().numpy(), d, ctx=ctx)
    sp._sh
    print(f"  host: validation, index build and upload {time.perf_counter() - t0:.2f} s, of which the index, row lists and work items "
          f"{sp.index_build_seconds():.2f} s", flush=True)

    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({ts.size} repetitions)", flush=True)
        return med

    def floor_ms(kk, rate, em):
        rec = kk * (kk + 1) // 2 + kk + 1
        per_entry = 12 + 8 * kk + ((12 + 8 * rec) if em else 0)
        return (nnz * per_entry + (n * 8.0 * rec if em else 8.0 * n)) / rate / 1e6

    hip = C.CDLL(_lib.LIB_PATH)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    if rows_mode:
        del rows, cols, vals
        nbytes = 1 << 32
        src, dst = torch.empty(nbytes // 8, dtype=torch.float64, device=dev), torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        def copy():
            assert hip.hipMemcpy(dst.data_ptr(), src.data_ptr(), C.c_size_t(nbytes), 3) == 0
            assert hip.hipDeviceSynchronize() == 0
        ks = [k] + ([int(sys.argv[sys.argv.index("--k2") + 1])] if "--k2" in sys.argv else [])
        models = {kk: P.PPCAModel.init(kk, sp, seed=3).iterate(sp) for kk in ks}
        legs = [("hipMemcpy device to device (4 GiB)", copy)]
        for kk in ks:
            legs += [(f"sparse llks, k = {kk}", lambda kk=kk: models[kk].llks(sp)), (f"sparse iterate, k = {kk}", lambda kk=kk: models[kk].iterate(sp))]
    else:
        xd = torch.full((n, d), float("nan"), dtype=torch.float64, device=dev)
        xd[mask] = vals
        del mask, rows, cols, vals
        torch.cuda.synchronize()
        dense = P.Dataset.from_device(xd.data_ptr(), n, d, ctx=ctx, keepalive=xd)
        spare = torch.empty((n, d), dtype=torch.float64, device=dev)
        nbytes = 8 * n * d
        def copy():
            assert hip.hipMemcpy(spare.data_ptr(), xd.data_ptr(), C.c_size_t(nbytes), 3) == 0
            assert hip.hipDeviceSynchronize() == 0
        ks = [k]
        model = P.PPCAModel.init(k, sp, seed=3).iterate(sp)
        legs = [("hipMemcpy device to device (N x d)", copy),
                ("PPCAModel.llks on to_dense()", lambda: model.llks(dense)), ("sparse llks", lambda: model.llks(sp)),
                ("PPCAModel.iterate on to_dense()", lambda: model.iterate(dense)), ("sparse iterate", lambda: model.iterate(sp))]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn))
    med = {name: report(name, np.concatenate(got[name])) for name, _ in legs}
    rate = 2.0 * nbytes / med[legs[0][0]] / 1e6  # GB/s of the copy (a read and a write)
    print(f"  copy rate {rate:.0f} GB/s")
    for kk in ks:
        tag = f", k = {kk}" if rows_mode else ""
        fl, fi = floor_ms(kk, rate, False), floor_ms(kk, rate, True)
        print(f"  k = {kk}: llks floor {fl:.3f} ms, achieved fraction {fl / med['sparse llks' + tag]:.3f};  iterate floor {fi:.3f} ms, "
              f"achieved fraction {fi / med['sparse iterate' + tag]:.3f}")
    if not rows_mode:
        print(f"  sparse / dense: llks {med['sparse llks'] / med['PPCAModel.llks on to_dense()']:.3f}, "
              f"iterate {med['sparse iterate'] / med['PPCAModel.iterate on to_dense()']:.3f}  (below 1: the sparse path is faster)")


def sparse_heldout_legs(reps=5, fraction=0.1):
    """Held-out scoring of a SparseDataset (`--sparse-heldout` beside `--sparse DENSITY` or `--sparse-rows M`), in one
    process, alternating, every repetition timed on its own: the host split (SparseDataset.holdout at `fraction`), heldout_score(train,
    held), sparse llks on train (the same row pass) and the composition the score replaces -- predict(train, held) and the numpy
    sums by row and by column.  The two device copies (index builds, uploads) are made once, before the timed legs."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    sp = P.SparseDataset(indptr, cols.int().cpu().numpy(), vals.cpu().numpy(), d, ctx=ctx)
    del cols, vals
    t0 = time.perf_counter()
    train, held = sp.holdout(fraction, 5)
    t_split = time.perf_counter() - t0
    t0 = time.perf_counter()
    train._sh, held._sh
    print(f"  held {held.nnz} of {nnz} entries ({held.nnz / nnz:.4f}); host: first split {t_split:.2f} s, index builds and uploads of the two "
          f"parts {time.perf_counter() - t0:.2f} s", flush=True)
    model = P.PPCAModel.init(k, train, seed=3).iterate(train)
    w = train.weights()

    def composition():
        mean, var = model.predict(train, held)
        hp, hc, hv = held._indptr, held._indices, held._values
        e = hv - mean
        e2 = e * e
        z2 = e2 / var
        l = -0.5 * (np.log(2.0 * np.pi) + np.log(var) + z2)
        rows = np.repeat(np.arange(n), np.diff(hp))
        per_row = np.bincount(rows, weights=l, minlength=n)
        we = w[rows]
        return per_row, [np.bincount(hc, weights=t, minlength=d) for t in (we, we * l, we * e2, we * z2)]

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({ts.size} repetitions)", flush=True)
        return med

    sc = model.heldout_score(train, held)
    per_row, sums = composition()
    print(f"  score {sc!r}; against the composition: per row {np.abs(sc.llks - per_row).max():.1e}, llk sum "
          f"{abs(sc.llk - sums[1].sum()) / abs(sc.llk):.1e} (relative)", flush=True)
    legs = [("host split (SparseDataset.holdout)", lambda: sp.holdout(fraction, 5), max(2, reps // 2), 0),
            ("heldout_score(train, held)", lambda: model.heldout_score(train, held), reps, 2),
            ("sparse llks on train", lambda: model.llks(train), reps, 2),
            ("predict(train, held) + numpy sums by row and column", composition, reps, 1)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn, r, warm in legs:
            got.setdefault(name, []).append(series(fn, r, warm))
    med = {name: report(name, np.concatenate(got[name])) for name, _, _, _ in legs}
    s, c_, l_ = med["heldout_score(train, held)"], med["predict(train, held) + numpy sums by row and column"], med["sparse llks on train"]
    print(f"  score / composition {s / c_:.3f} (below 1: the score is faster);  score / llks {s / l_:.3f}")


def sparse_topn_legs(reps=5):
    """PPCAModel.recommend on a SparseDataset (`--sparse-topn N_TOP [--n2 N2] [--kappa KAPPA] [--slice ROWS] [--reps R]` beside
    `--sparse DENSITY` or `--sparse-rows M`), in one process, alternating, every repetition timed on its own: sparse llks (the row pass
    the call shares), recommend at N_TOP (and at N2, and at N_TOP with KAPPA), and what the call replaces -- predict at all positions of
    a slice of ROWS rows (default: 2^24 positions) and np.argpartition, scaled to N.  Floor (a): N d k multiply-adds (N d (k^2 + 2 k)
    with kappa) at 78.6 TFLOP/s, plus the llks time."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    sp = P.SparseDataset(indptr, cols.int().cpu().numpy(), vals.cpu().numpy(), d, ctx=ctx)
    del cols, vals
    sp._sh
    n_top = int(sys.argv[sys.argv.index("--sparse-topn") + 1])
    tops = [(n_top, 0.0)]
    if "--n2" in sys.argv:
        tops.append((int(sys.argv[sys.argv.index("--n2") + 1]), 0.0))
    if "--kappa" in sys.argv:
        tops.append((n_top, float(sys.argv[sys.argv.index("--kappa") + 1])))
    rows = int(sys.argv[sys.argv.index("--slice") + 1]) if "--slice" in sys.argv else max(1, min(n, (1 << 24) // d))
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    model = P.PPCAModel.init(k, sp, seed=3).iterate(sp)
    q_indptr = np.zeros(n + 1, dtype=np.int64)
    q_indptr[1:rows + 1] = d
    q_indptr = np.cumsum(q_indptr)
    q_cols = np.tile(np.arange(d, dtype=np.int32), rows)

    def composition():
        mean, _ = model.predict(sp, (q_indptr, q_cols))
        mean = mean.reshape(rows, d)
        mean[np.repeat(np.arange(rows), np.diff(indptr[:rows + 1])), sp._indices[:indptr[rows]]] = -np.inf
        return np.argpartition(mean, d - min(n_top, d), axis=1)[:, d - min(n_top, d):]

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({ts.size} repetitions)", flush=True)
        return med

    got_cols, _ = model.recommend(sp, n_top)
    want = np.sort(composition(), axis=1)
    same = float(np.mean(np.sort(got_cols[:rows], axis=1) == want)) if n_top <= d else float("nan")
    print(f"  recommend against the composition on the first {rows} rows: {same:.6f} of the columns agree (ties and last bits apart)", flush=True)
    name_of = lambda t, kap: f"recommend n = {t}" + (f", kappa = {kap:g}" if kap else "")
    legs = [("sparse llks", lambda: model.llks(sp), reps, 2)]
    legs += [(name_of(t, kap), lambda t=t, kap=kap: model.recommend(sp, t, kappa=kap), reps, 2) for t, kap in tops]
    legs += [(f"predict at all positions of {rows} rows + argpartition", composition, reps, 1)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn, r, warm in legs:
            got.setdefault(name, []).append(series(fn, r, warm))
    med = {name: report(name, np.concatenate(got[name])) for name, _, _, _ in legs}
    comp = med[legs[-1][0]] * n / rows
    for t, kap in tops:
        fl = 2.0 * n * d * (k * k + 2 * k if kap else k) / 78.6e12 * 1e3
        m = med[name_of(t, kap)]
        print(f"  {name_of(t, kap)}: floor {fl:.3f} ms + llks {med['sparse llks']:.3f} ms = {fl + med['sparse llks']:.3f} ms, achieved fraction "
              f"{(fl + med['sparse llks']) / m:.3f} (of the ranking alone: {fl / max(m - med['sparse llks'], 1e-9):.3f});  the composition scaled "
              f"to N: {comp / 1e3:.1f} s = {comp / m:.0f} x")


def sparse_mix_legs(nm, reps=5):
    """PPCAMix on a SparseDataset (`--mix NM [--reps R]` beside `--sparse DENSITY` or `--sparse-rows M`), in one process,
    alternating, every repetition timed on its own, NM components of state size K: (a) the fused row pass (the component-major ell
    buffer, downloaded: NM x N doubles) against NM calls of PPCAModel.llks (the single-model row pass; N doubles downloaded each, plus
    its scalar sums); (b) one PPCAMix.iterate against NM x PPCAModel.iterate; (c) PPCAMix.predict at 1 M query entries against NM x
    PPCAModel.predict."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    sp = P.SparseDataset(indptr, cols.int().cpu().numpy(), vals.cpu().numpy(), d, ctx=ctx)
    del cols, vals
    sp._sh
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    mix = P.PPCAMix.init(nm, k, sp, seed=3).iterate(sp)
    models = mix.models
    devs, arr = mix._handles(ctx)
    ell = np.empty((nm, n))
    rng = np.random.default_rng(5)
    nq = 1 << 20
    q_indptr = np.searchsorted(np.sort(rng.integers(0, n, nq)), np.arange(n + 1), side="left").astype(np.int64)
    q_cols = rng.integers(0, d, nq).astype(np.int32)

    def fused():
        _lib.check(_lib.lib().ppca_mix_sparse_component_llks(ctx.handle, sp._sh, arr, nm, _lib.ptr(ell)))

    def series(fn, r, warm=2):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({ts.size} repetitions)", flush=True)
        return med

    fused()
    same = all(np.array_equal(ell[c], m.llks(sp)) for c, m in enumerate(models))
    print(f"  the fused pass's ell against PPCAModel.llks, component by component: {'bit-identical' if same else 'DIFFERENT'}", flush=True)
    legs = [(f"(a) fused row pass, {nm} components", fused),
            (f"(a) {nm} x PPCAModel.llks", lambda: [m.llks(sp) for m in models]),
            ("(b) PPCAMix.iterate", lambda: mix.iterate(sp)),
            (f"(b) {nm} x PPCAModel.iterate", lambda: [m.iterate(sp) for m in models]),
            (f"(c) PPCAMix.predict, {nq} entries", lambda: mix.predict(sp, (q_indptr, q_cols))),
            (f"(c) {nm} x PPCAModel.predict", lambda: [m.predict(sp, (q_indptr, q_cols)) for m in models])]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn, reps))
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    spread = [float(np.ptp(np.concatenate(got[name])) / np.median(np.concatenate(got[name]))) for name, _ in legs]
    for i, what in ((0, "fused / separate row passes"), (2, "mixture iterate / nm single iterates"), (4, "mixture predict / nm single predicts")):
        print(f"  {what}: {med[i] / med[i + 1]:.3f}  (run-to-run spread of the two legs: {spread[i]:.1%}, {spread[i + 1]:.1%})", flush=True)


def sparse_mix_topn_legs(nm, reps=5):
    """PPCAMix.recommend on a SparseDataset (`--sparse-topn N_TOP --mix NM [--kappa KAPPA] [--slice ROWS] [--reps R]` beside
    `--sparse DENSITY` or `--sparse-rows M`), in one process, alternating, every repetition timed on its own, NM components of state
    size K: (a) PPCAMix.recommend at N_TOP (with KAPPA when given); (b) NM x PPCAModel.recommend, the same multiply-adds with NM lists
    and NM downloads; (c) the floor: NM N d k multiply-adds (NM N d (k^2 + 2 k) with kappa) at 78.6 TFLOP/s plus the mixture's ell
    pass (PPCAMix.llks); (d) what the call replaces -- PPCAMix.predict at all positions of a slice of ROWS rows (default: 2^24
    positions) and np.argpartition, scaled to N."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    sp = P.SparseDataset(indptr, cols.int().cpu().numpy(), vals.cpu().numpy(), d, ctx=ctx)
    del cols, vals
    sp._sh
    n_top = int(sys.argv[sys.argv.index("--sparse-topn") + 1])
    kap = float(sys.argv[sys.argv.index("--kappa") + 1]) if "--kappa" in sys.argv else 0.0
    rows = int(sys.argv[sys.argv.index("--slice") + 1]) if "--slice" in sys.argv else max(1, min(n, (1 << 24) // d))
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    mix = P.PPCAMix.init(nm, k, sp, seed=3).iterate(sp)
    models = mix.models
    q_indptr = np.zeros(n + 1, dtype=np.int64)
    q_indptr[1:rows + 1] = d
    q_indptr = np.cumsum(q_indptr)
    q_cols = np.tile(np.arange(d, dtype=np.int32), rows)

    def composition():
        mean, var = mix.predict(sp, (q_indptr, q_cols))
        score = (mean + kap * np.sqrt(var) if kap else mean).reshape(rows, d)
        score[np.repeat(np.arange(rows), np.diff(indptr[:rows + 1])), sp._indices[:indptr[rows]]] = -np.inf
        return np.argpartition(score, d - min(n_top, d), axis=1)[:, d - min(n_top, d):]

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({ts.size} repetitions)", flush=True)
        return med

    got_cols, _ = mix.recommend(sp, n_top, kappa=kap)
    want = np.sort(composition(), axis=1)
    same = float(np.mean(np.sort(got_cols[:rows], axis=1) == want)) if n_top <= d else float("nan")
    print(f"  recommend against the composition on the first {rows} rows: {same:.6f} of the columns agree (ties and last bits apart)", flush=True)
    tag = f"n = {n_top}" + (f", kappa = {kap:g}" if kap else "")
    legs = [(f"(a) PPCAMix.recommend {tag}, {nm} components", lambda: mix.recommend(sp, n_top, kappa=kap), reps, 2),
            (f"(b) {nm} x PPCAModel.recommend {tag}", lambda: [m.recommend(sp, n_top, kappa=kap) for m in models], reps, 2),
            ("(c) PPCAMix.llks (the mixture's ell pass)", lambda: mix.llks(sp), reps, 2),
            (f"(d) PPCAMix.predict at all positions of {rows} rows + argpartition", composition, reps, 1)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn, r, warm in legs:
            got.setdefault(name, []).append(series(fn, r, warm))
    med = [report(name, np.concatenate(got[name])) for name, _, _, _ in legs]
    spread = [float(np.ptp(np.concatenate(got[name])) / np.median(np.concatenate(got[name]))) for name, _, _, _ in legs]
    fl = 2.0 * nm * n * d * (k * k + 2 * k if kap else k) / 78.6e12 * 1e3
    comp = med[3] * n / rows
    print(f"  (a) / (b): {med[0] / med[1]:.3f} (below 1: the fused call is faster; run-to-run spread of the two legs: {spread[0]:.1%}, {spread[1]:.1%})")
    print(f"  (c) floor {fl:.3f} ms + ell pass {med[2]:.3f} ms = {fl + med[2]:.3f} ms, achieved fraction {(fl + med[2]) / med[0]:.3f} (of the ranking "
          f"alone: {fl / max(med[0] - med[2], 1e-9):.3f})")
    print(f"  (d) the composition scaled to N: {comp / 1e3:.1f} s;  (d) / (a): {comp / med[0]:.0f} x (spread of (d): {spread[3]:.1%})")


def sparse_fa_legs(reps=5):
    """FAModel on a SparseDataset (`--fa [--reps R]` beside `--sparse DENSITY` or `--sparse-rows M`), in one process,
    alternating, every repetition timed on its own: (a) ppca_scale_columns_sparse with the view and the column sums, (b) its sums-only
    form, (c) PPCAModel.iterate(sp), (d) FAModel.iterate(sp), and (e) what there was before the scale pass: a new SparseDataset from
    the rescaled host values (validation, index build, upload) plus PPCAModel.iterate on it -- one repetition per round, it takes
    seconds.  Reported: (d) / (c), (a) / (c), and the bytes per second of (a) at 36 B per entry (both orientations: 8 B read, 8 B
    written; the 4 B column index of the CSR copy; the a[col] gather stays in cache; the data carries no weights, so the row index of
    the inverted copy is not read) and of (b) at 8 B per entry."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    ix, v = cols.int().cpu().numpy(), vals.cpu().numpy()
    del cols, vals
    sp = P.SparseDataset(indptr, ix, v, d, ctx=ctx)
    sp._sh
    print(f"  host: the index, row lists and work items {sp.index_build_seconds():.2f} s", flush=True)
    model = P.PPCAModel.init(k, sp, seed=3).iterate(sp)
    rng = np.random.default_rng(5)
    fa = P.FAModel(model.isotropic_noise * rng.uniform(0.5, 2.0, d), model.transform, model.mean)
    a, b = 1.0 / fa.noise, fa.mean / fa.noise

    def scale():
        sp._scale_columns(a, b, col_sums=True)

    def sums():
        sp._scale_columns(a, b, out=False, col_sums=True)

    def rebuild():
        model.iterate(P.SparseDataset(indptr, ix, v * a[ix], d, ctx=ctx))

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:72s} median {med:10.3f} ms  min {ts.min():10.3f}  max {ts.max():10.3f}  ({ts.size} repetitions)", flush=True)
        return med

    legs = [("(a) scale pass: view + column sums", scale, reps, 2), ("(b) scale pass: column sums only", sums, reps, 2),
            ("(c) PPCAModel.iterate(sp)", lambda: model.iterate(sp), reps, 2), ("(d) FAModel.iterate(sp)", lambda: fa.iterate(sp), reps, 2),
            ("(e) new SparseDataset from rescaled host values + PPCAModel.iterate", rebuild, 1, 0)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn, r, warm in legs:
            got.setdefault(name, []).append(series(fn, r, warm))
    med = [report(name, np.concatenate(got[name])) for name, _, _, _ in legs]
    spread = [float((np.concatenate(got[name]).max() - np.concatenate(got[name]).min()) / m_) for (name, _, _, _), m_ in zip(legs, med)]
    print(f"  (d) / (c): {med[3] / med[2]:.3f};  (a) / (c): {med[0] / med[2]:.3f};  (e) / (d): {med[4] / med[3]:.1f} x  "
          f"(run-to-run spread of (c), (d): {spread[2]:.1%}, {spread[3]:.1%})")
    print(f"  (a) {36.0 * nnz / med[0] / 1e6:.0f} GB/s at 36 B per entry;  (b) {8.0 * nnz / med[1] / 1e6:.0f} GB/s at 8 B per entry")


def sparse_t_legs(reps=5):
    """TPPCAModel on a SparseDataset (`--robust [--reps R]` beside `--sparse DENSITY` or `--sparse-rows M`), in one
    process, alternating, every repetition timed on its own behind a synchronise: (1) PPCAModel.llks(sp), (2) TPPCAModel.llks(sp),
    (3) the E-step with the view and the column sums, (4) PPCAModel.iterate(sp), (5) TPPCAModel.iterate(sp).  The yardstick is the
    Gaussian model's own passes in the same process: reported are (2) / (1), (3) / (4) and (5) / (4)."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    ix, v = cols.int().cpu().numpy(), vals.cpu().numpy()
    del cols, vals
    sp = P.SparseDataset(indptr, ix, v, d, ctx=ctx)
    sp._sh
    print(f"  host: the index, row lists and work items {sp.index_build_seconds():.2f} s", flush=True)
    model = P.PPCAModel.init(k, sp, seed=3).iterate(sp)
    t = P.TPPCAModel.from_ppca(model, 4.0, row_compressed=True)

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:72s} median {med:10.3f} ms  min {ts.min():10.3f}  max {ts.max():10.3f}  ({ts.size} repetitions)", flush=True)
        return med

    legs = [("(1) PPCAModel.llks(sp)", lambda: model.llks(sp)), ("(2) TPPCAModel.llks(sp)", lambda: t.llks(sp)),
            ("(3) t E-step: view + column sums", lambda: t._estep(sp, scaled=True, col_sums=True, scalars=True)),
            ("(4) PPCAModel.iterate(sp)", lambda: model.iterate(sp)), ("(5) TPPCAModel.iterate(sp)", lambda: t.iterate(sp))]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn, reps, 2))
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    spread = [float((np.concatenate(got[name]).max() - np.concatenate(got[name]).min()) / m_) for (name, _), m_ in zip(legs, med)]
    print(f"  (2) / (1): {med[1] / med[0]:.3f};  (3) / (4): {med[2] / med[3]:.3f};  (5) / (4): {med[4] / med[3]:.3f}  "
          f"(run-to-run spread of (4), (5): {spread[3]:.1%}, {spread[4]:.1%});  (1) + (3) + (4) = {med[0] + med[2] + med[3]:.3f} ms "
          f"against (5) = {med[4]:.3f} ms")


def sparse_h_legs(reps=5):
    """HPPCAModel on a SparseDataset (`--sparse-h [--reps R]` beside `--sparse DENSITY` or `--sparse-rows M`), in one
    process, alternating, every repetition timed on its own behind a synchronise: (1) PPCAModel.llks(sp), (2) HPPCAModel.llks(sp, view),
    (3) the construction of the precisions' view (host check, upload of nnz doubles, the fill of the index-order copy),
    (4) PPCAModel.iterate(sp), (5) HPPCAModel.iterate(sp, view).  Precisions log-uniform in [2^-10, 2^10].  The yardstick is the
    Gaussian model's own passes in the same process: reported are (2) / (1), (3) / (4) and (5) / (4)."""
    _, _, _, _, cols, vals, _, indptr, nnz = sparse_data()
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    ix, v = cols.int().cpu().numpy(), vals.cpu().numpy()
    del cols, vals
    sp = P.SparseDataset(indptr, ix, v, d, ctx=ctx)
    sp._sh
    print(f"  host: the index, row lists and work items {sp.index_build_seconds():.2f} s", flush=True)
    model = P.PPCAModel.init(k, sp, seed=3).iterate(sp)
    h = P.HPPCAModel.from_ppca(model, row_compressed=True)
    pv = np.exp(np.random.default_rng(9).uniform(np.log(2.0 ** -10), np.log(2.0 ** 10), nnz))
    view = h._sparse_pair(sp, pv)

    def series(fn, r, warm):
        for _ in range(warm):
            fn()
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:72s} median {med:10.3f} ms  min {ts.min():10.3f}  max {ts.max():10.3f}  ({ts.size} repetitions)", flush=True)
        return med

    legs = [("(1) PPCAModel.llks(sp)", lambda: model.llks(sp)), ("(2) HPPCAModel.llks(sp, view)", lambda: h.llks(sp, view)),
            ("(3) the precisions' view: check, upload, index-order fill", lambda: h._sparse_pair(sp, pv)),
            ("(4) PPCAModel.iterate(sp)", lambda: model.iterate(sp)), ("(5) HPPCAModel.iterate(sp, view)", lambda: h.iterate(sp, view))]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn, reps, 2))
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    spread = [float((np.concatenate(got[name]).max() - np.concatenate(got[name]).min()) / m_) for (name, _), m_ in zip(legs, med)]
    print(f"  (2) / (1): {med[1] / med[0]:.3f};  (3) / (4): {med[2] / med[3]:.3f};  (5) / (4): {med[4] / med[3]:.3f}  "
          f"(run-to-run spread of (4), (5): {spread[3]:.1%}, {spread[4]:.1%})")


def sparse_build_legs(reps=2):
    """The device-side build of SparseDataset (`--sparse-build [--reps R]` beside `--sparse DENSITY` or
    `--sparse-rows M`), in one process, alternating, every repetition timed on its own behind a synchronise, host path against device
    path: (1) ppca_sparse_from_host (validation, index, row lists, work items, upload of five arrays) from host arrays, (2)
    SparseDataset.from_device from the same arrays resident on the device; (3) the host holdout(0.1) and the device copies of both
    parts, (4) the device split of the device-born dataset; (5), (6) PPCATrainer.select_state_size([K], folds=5, n_iters=5) on the
    host-born and on the device-born dataset.  Reported: the medians and (2) / (1), (4) / (3), (6) / (5)."""
    torch, dev, _, _, cols, vals, _, indptr, nnz = sparse_data()
    if "--reps" in sys.argv:
        reps = int(sys.argv[sys.argv.index("--reps") + 1])
    ip_d, ix_d, v_d = torch.from_numpy(indptr).to(dev), cols.int().contiguous(), vals.contiguous()
    ix, v = ix_d.cpu().numpy(), v_d.cpu().numpy()
    del cols, vals
    torch.cuda.synchronize()
    host = P.SparseDataset(indptr, ix, v, d, ctx=ctx)

    def host_build():
        s = P.SparseDataset.__new__(P.SparseDataset)  # (the same arrays, no second pass of the Python checks)
        s.__dict__.update(host.__dict__)
        s._handle = None
        s._sh
        return s

    def dev_build():
        return P.SparseDataset.from_device(ip_d.data_ptr(), ix_d.data_ptr(), v_d.data_ptr(), n, d, ctx=ctx, keepalive=(ip_d, ix_d, v_d))

    host._sh
    born = dev_build()
    print(f"  index, row lists and work items: host {host.index_build_seconds():.3f} s (without validation and upload), device "
          f"{born.index_build_seconds():.3f} s (with validation and waits)", flush=True)

    def host_split():
        t, h = host.holdout(0.1, 5)
        t._sh, h._sh

    def select(sp):
        return P.PPCATrainer(sp).select_state_size([k], seed=7, folds=5, n_iters=5)

    def series(fn, r):
        ctx.synchronize()
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:72s} median {med:10.2f} ms  min {ts.min():10.2f}  max {ts.max():10.2f}  ({ts.size} repetitions)", flush=True)
        return med

    a, b = select(host), select(born)  # (also the warm-up: code objects, the block cache)
    print(f"  select_state_size mean_llk: host-born {a[0][1].mean_llk!r}, device-born {b[0][1].mean_llk!r}", flush=True)
    legs = [("(1) host build and upload (ppca_sparse_from_host)", host_build, reps), ("(2) device build (SparseDataset.from_device)", dev_build, reps),
            ("(3) host holdout(0.1) and the device copies of both parts", host_split, reps),
            ("(4) device split (holdout(0.1) of the device-born dataset)", lambda: born.holdout(0.1, 5), reps),
            (f"(5) select_state_size([{k}], folds=5, n_iters=5), host-born", lambda: select(host), 1),
            (f"(6) select_state_size([{k}], folds=5, n_iters=5), device-born", lambda: select(born), 1)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn, r in legs:
            got.setdefault(name, []).append(series(fn, r))
    med = [report(name, np.concatenate(got[name])) for name, _, _ in legs]
    print(f"  nnz = {nnz}: (2) / (1): {med[1] / med[0]:.3f};  (4) / (3): {med[3] / med[2]:.3f};  (6) / (5): {med[5] / med[4]:.3f}  "
          "(below 1: the device path is faster)")


if "--sparse-build" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_build_legs()
    sys.exit(0)
if "--sparse-h" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_h_legs()
    sys.exit(0)
if "--robust" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_t_legs()
    sys.exit(0)
if "--fa" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_fa_legs()
    sys.exit(0)
if "--mix" in sys.argv and "--sparse-topn" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_mix_topn_legs(int(sys.argv[sys.argv.index("--mix") + 1]))
    sys.exit(0)
if "--mix" in sys.argv and ("--sparse" in sys.argv or "--sparse-rows" in sys.argv):
    sparse_mix_legs(int(sys.argv[sys.argv.index("--mix") + 1]))
    sys.exit(0)
if "--sparse-topn" in sys.argv:
    sparse_topn_legs()
    sys.exit(0)
if "--sparse-heldout" in sys.argv:
    sparse_heldout_legs()
    sys.exit(0)
if "--sparse" in sys.argv or "--sparse-rows" in sys.argv:
    sparse_legs()
    sys.exit(0)

truth = P.PPCAModel(0.1, np.random.default_rng(1).standard_normal((d, k)), np.random.default_rng(2).standard_normal(d))
spec = _lib.SynthSpec(0, n, d, k, 0.1, 0.3, 0, 0, 1033, truth._c.ctypes.data_as(_lib.c_double_p),
                      truth._mean.ctypes.data_as(_lib.c_double_p))
h = C.c_void_p()
_lib.check(_lib.lib().ppca_dataset_generate(ctx.handle, C.byref(spec), C.byref(h)))
ds = P.Dataset._wrap(h, ctx)
m = P.PPCAModel.init(k, ds, seed=3).iterate(ds).iterate(ds)
L = _lib.lib()
md = m._device(ctx)

def fa_legs(reps=12):
    hip = C.CDLL(_lib.LIB_PATH)  # (dlsym on the library's handle reaches the HIP runtime it is bound to)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []

    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts, nbytes):
        med = float(np.median(ts))
        print(f"{name:44s} median {med:8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  max/median {ts.max()/med:5.3f}  "
              f"{nbytes/med/1e6:8.1f} GB/s  ({reps} repetitions)", flush=True)
        return med

    rng = np.random.default_rng(5)
    a, b = rng.uniform(0.5, 2.0, d), rng.standard_normal(d)
    sums = np.empty((3, d))
    nd_bytes = 8.0 * n * d
    dst = C.c_void_p()
    _lib.check(L.ppca_dataset_scale_columns(ctx.handle, ds._h, _lib.ptr(a), None, None, C.byref(dst), None, None))
    src_p, dst_p = L.ppca_dataset_device_x(ds._h), L.ppca_dataset_device_x(dst)
    def copy():
        assert hip.hipMemcpy(dst_p, src_p, C.c_size_t(int(nd_bytes)), 3) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0
    def scale(with_out):
        o = C.c_void_p()
        _lib.check(L.ppca_dataset_scale_columns(ctx.handle, ds._h, _lib.ptr(a), _lib.ptr(b), None, C.byref(o) if with_out else None,
                                                _lib.ptr(sums), None))
        if with_out:
            L.ppca_dataset_free(o)
    # the copy and the pass alternate, so that both see the same machine
    t_copy, t_scale = [], []
    for _ in range(2):
        t_copy.append(series(copy)); t_scale.append(series(lambda: scale(True)))
    t_copy, t_scale = np.concatenate(t_copy), np.concatenate(t_scale)
    reps *= 2
    c = report("hipMemcpy device to device (N x d)", t_copy, 2 * nd_bytes)
    s1 = report("scale pass with output (+ column sums)", t_scale, 2 * nd_bytes + 8.0 * n)
    print(f"  scale pass / copy = {s1 / c:.3f}   (the copy's own spread, max / median: {t_copy.max() / c:.3f})")
    reps //= 2
    s0 = report("scale pass, sums only (no N x d output)", series(lambda: scale(False)), nd_bytes)
    print(f"  sums only / read half of the copy = {s0 / (c / 2):.3f}")
    L.ppca_dataset_free(dst)
    # one FA iteration against one PPCA iteration (ppca_em_step), both from the model m
    out = C.c_void_p()
    _lib.check(L.ppca_model_alloc(ctx.handle, d, k, C.byref(out)))
    llk = C.c_double()
    t_pp = series(lambda: _lib.check(L.ppca_em_step(ctx.handle, ds._h, md.h, None, out, C.byref(llk))))
    L.ppca_model_free(out)
    fa = P.FAModel.from_ppca(m)
    no, co, mo = np.empty(d), np.empty((d, k)), np.empty(d)
    t_fa = series(lambda: _lib.check(L.ppca_fa_em_step(ctx.handle, ds._h, d, k, _lib.ptr(fa._noise), _lib.ptr(fa._c), _lib.ptr(fa._mean), None,
                                                       _lib.ptr(no), _lib.ptr(co), _lib.ptr(mo), C.byref(llk))))
    pp = report("PPCA iteration (ppca_em_step, llk read)", t_pp, nd_bytes)
    ff = report("FA iteration (ppca_fa_em_step, llk read)", t_fa, 3 * nd_bytes)
    print(f"  FA / PPCA = {ff / pp:.3f}   (FA - PPCA = {ff - pp:.3f} ms; the scale pass alone: {s1:.3f} ms)")

if "--fa" in sys.argv:
    fa_legs()
    sys.exit(0)

def robust_legs(reps=10):
    """The Student-t sweep with and without the scaled rows, a whole TPPCAModel.iterate, and in the same process the
    passes whose traffic the sweep adds up to (two reads and one write of N x d): PPCAModel.llks, the column-scale pass with output and
    sums, and PPCAModel.iterate.  Every repetition timed on its own (median, min, max)."""
    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  ({reps} repetitions)", flush=True)
        return med

    t = P.TPPCAModel.from_ppca(m, 4.0)
    a, b = np.ones(d), m.mean
    legs = [("PPCAModel.llks (posterior pass, llks to the host)", lambda: m.llks(ds)),
            ("scale pass with output and column sums", lambda: ds._scale_columns(a, b, out=True, col_sums=True)),
            ("t sweep without the scaled rows (llks to the host)", lambda: t.llks(ds)),
            ("t sweep with the scaled rows and column sums", lambda: t._estep(ds, scaled=True, col_sums=True, scalars=True)),
            ("PPCAModel.iterate", lambda: m.iterate(ds)),
            ("TPPCAModel.iterate", lambda: t.iterate(ds))]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn))
    reps *= 2
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    print(f"  sweep without Y / llks = {med[2] / med[0]:.3f}   (the sweep alone: {med[2] - med[0]:.3f} ms)")
    print(f"  sweep with Y / (llks + scale) = {med[3] / (med[0] + med[1]):.3f}   (the sweep alone: {med[3] - med[0]:.3f} ms; scale pass {med[1]:.3f} ms)")
    print(f"  t iterate / Gaussian iterate = {med[5] / med[4]:.3f}   (t - Gaussian = {med[5] - med[4]:.3f} ms)")

if "--robust" in sys.argv:
    robust_legs()
    sys.exit(0)

def heldout_legs(reps=10, fraction=0.1):
    """Held-out scoring, in one process and alternating: the device split (Dataset.holdout), the score
    (PPCAModel.heldout_score on the two parts), PPCAModel.loo_llks on the same data (the same posterior pass, the k^2 work on every
    entry), the column-scale pass with output (two of the split's three array streams), and the composition the feature replaces:
    extrapolate + extrapolated_covariances_diagonal of the train part and both downloads.  Every repetition timed on its own."""
    def series(fn, r):
        fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  ({len(ts)} repetitions)", flush=True)
        return med

    train, held = ds.holdout(fraction, 11)
    print(f"split: kept {train.holdout_counts[0]}, held {train.holdout_counts[1]} "
          f"(share {train.holdout_counts[1] / max(sum(train.holdout_counts), 1):.5f})", flush=True)
    a = np.ones(d)

    def composition():  # (the diagonal through the device pass, ppca_covariance_diagonal mode 1: the faster of the two public routes)
        o = C.c_void_p()
        _lib.check(L.ppca_covariance_diagonal(ctx.handle, train._h, md.h, 1, C.byref(o)))
        return m.extrapolate(train).numpy(), P.Dataset._wrap(o, ctx).numpy()

    legs = [("Dataset.holdout (one read, two writes, counts)", lambda: ds.holdout(fraction, 11)),
            ("PPCAModel.heldout_score (train, held)", lambda: m.heldout_score(train, held)),
            ("PPCAModel.loo_llks (train + held rows = the dataset)", lambda: m.loo_llks(ds)),
            ("scale pass with output", lambda: ds._scale_columns(a, out=True)),
            ("extrapolate + covariance diagonal + both downloads", composition)]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn, reps))
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    print(f"  split / scale pass with output = {med[0] / med[3]:.3f}   (three array streams against two: 1.5 expected)")
    print(f"  score / loo_llks = {med[1] / med[2]:.3f}")
    print(f"  composition / (split + score) = {med[4] / (med[0] + med[1]):.1f}")

if "--heldout" in sys.argv:
    heldout_legs()
    sys.exit(0)

def hetero_legs(reps=10):
    """HPPCAModel against PPCAModel on the same rows: precisions log-uniform in [2^-10, 2^10] with 10 % zeros and 5 %
    NaN, made on the device.  Every repetition timed on its own (median, min, max); the legs alternate."""
    import torch

    hip = C.CDLL(_lib.LIB_PATH)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []

    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:60s} median {med:8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  ({reps} repetitions)", flush=True)
        return med

    torch.manual_seed(7)
    pt = torch.empty((n, d), dtype=torch.float64, device="cuda").uniform_(-10.0 * np.log(2.0), 10.0 * np.log(2.0)).exp_()
    u = torch.rand((n, d), device="cuda")
    pt[u < 0.10] = 0.0
    pt[(u >= 0.10) & (u < 0.15)] = float("nan")
    del u
    torch.cuda.synchronize()
    prec = P.Dataset.from_device(pt.data_ptr(), n, d, ctx=ctx, keepalive=pt)
    hm = P.HPPCAModel.from_ppca(m)
    nd_bytes = 8.0 * n * d
    spare = torch.empty((n, d), dtype=torch.float64, device="cuda")
    src_p, dst_p = L.ppca_dataset_device_x(ds._h), spare.data_ptr()
    def copy():
        assert hip.hipMemcpy(dst_p, src_p, C.c_size_t(int(nd_bytes)), 3) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0
    legs = [("hipMemcpy device to device (N x d)", copy),
            ("PPCAModel.llks (llks to the host)", lambda: m.llks(ds)),
            ("HPPCAModel.llks (the sweep alone, llks to the host)", lambda: hm.llks(ds, prec)),
            ("PPCAModel.iterate", lambda: m.iterate(ds)),
            ("HPPCAModel.iterate", lambda: hm.iterate(ds, prec))]
    got = {}
    for _ in range(2):  # the legs alternate, so that all see the same machine
        for name, fn in legs:
            got.setdefault(name, []).append(series(fn))
    reps *= 2
    med = [report(name, np.concatenate(got[name])) for name, _ in legs]
    rate = 2 * nd_bytes / med[0] / 1e6  # GB/s of the copy (a read and a write)
    rec = k * (k + 1) // 2 + k + 1
    rec_pad = 16 * ((rec + 15) // 16)
    floor_sweep = 2 * nd_bytes / rate / 1e6
    floor_iter = (4 * nd_bytes + 2 * 8.0 * n * rec) / rate / 1e6
    print(f"  copy rate {rate:.0f} GB/s; record {rec} doubles per row ({rec_pad} as stored)")
    print(f"  sweep: floor (X and P once) {floor_sweep:.3f} ms, achieved fraction {floor_sweep / med[2]:.3f};  sweep / PPCAModel.llks = {med[2] / med[1]:.3f}")
    print(f"  iterate: floor (X and P twice, records once each way) {floor_iter:.3f} ms, achieved fraction {floor_iter / med[4]:.3f}")
    print(f"  HPPCAModel.iterate / PPCAModel.iterate = {med[4] / med[3]:.3f}   (the statistics contraction and the rest: {med[4] - med[2]:.3f} ms)")

if "--hetero" in sys.argv:
    hetero_legs()
    sys.exit(0)

def famix_legs(nm, reps=12):
    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts, nbytes=None):
        med = float(np.median(ts))
        rate = f"{nbytes/med/1e6:8.1f} GB/s" if nbytes else " " * 13
        print(f"{name:52s} median {med:8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  {rate}  ({reps} repetitions)", flush=True)
        return med

    rng = np.random.default_rng(5)
    a, b = rng.uniform(0.5, 2.0, d), rng.standard_normal(d)
    sums = np.empty((3, d))
    def scale(with_out):
        o = C.c_void_p()
        _lib.check(L.ppca_dataset_scale_columns(ctx.handle, ds._h, _lib.ptr(a), _lib.ptr(b), None, C.byref(o) if with_out else None,
                                                _lib.ptr(sums), None))
        if with_out:
            L.ppca_dataset_free(o)
    # K x n weights on the device: in [0, 1], most of a row's weight in few components, as exp-shifted responsibilities are
    e = rng.uniform(0.0, 1.0, (nm * n, 1)) ** 4
    E = P.Dataset(e)
    del e
    e_dev = L.ppca_dataset_device_x(E._h)
    bm = np.ascontiguousarray(rng.standard_normal((nm, d)))
    msums = np.empty((nm, 3, d))
    def sweep():
        _lib.check(L.ppca_dataset_column_moments_multi(ctx.handle, ds._h, None, C.c_void_p(e_dev), nm, _lib.ptr(a), _lib.ptr(bm), _lib.ptr(msums)))
    t_a, t_b = [], []
    for _ in range(2):  # the two sweeps alternate, so that both see the same machine
        t_a.append(series(lambda: scale(False))); t_b.append(series(sweep))
    t_a, t_b = np.concatenate(t_a), np.concatenate(t_b)
    reps *= 2
    ta = report("(a) scale pass, sums only", t_a, 8.0 * n * d)
    tb = report(f"(b) multi-component sweep, K = {nm}", t_b, n * (8.0 * d + 8.0 * nm))
    print(f"  (b) / (a) = {tb / ta:.3f}   (the {nm} separate sweeps it replaces: {nm} x (a) = {nm * ta:.3f} ms, {nm * ta / tb:.2f} x (b))")
    reps //= 2
    tw = report("whitening: scale pass with output (+ sums)", series(lambda: scale(True)), 16.0 * n * d)
    del E
    # the two mixture iterations from the same components: perturbed copies of m, as the --mix leg
    comps = [P.PPCAModel(1.0, m.transform + 0.1 * rng.standard_normal((d, k)), m.mean) for _ in range(nm)]
    mix = P.PPCAMix(comps, np.full(nm, -np.log(nm)))
    devs, arr = mix._handles(ctx)
    outs = []
    for _ in range(nm):
        hh = C.c_void_p()
        _lib.check(L.ppca_model_alloc(ctx.handle, d, k, C.byref(hh)))
        outs.append(hh)
    oarr = (C.c_void_p * nm)(*outs)
    lw_out, llk = np.empty(nm), C.c_double()
    t_c = series(lambda: _lib.check(L.ppca_mix_em_step(ctx.handle, ds._h, arr, _lib.ptr(mix._lw), nm, None, oarr, _lib.ptr(lw_out), C.byref(llk))))
    for hh in outs:
        L.ppca_model_free(hh)
    fm = P.FAMix.from_ppca_mix(mix)
    no, co, mo = np.empty(d), np.empty((nm, d, k)), np.empty((nm, d))
    t_d = series(lambda: _lib.check(L.ppca_famix_em_step(ctx.handle, ds._h, d, k, nm, _lib.ptr(fm._noise), _lib.ptr(fm._c), _lib.ptr(fm._mean),
                                                         _lib.ptr(fm._lw), None, _lib.ptr(no), _lib.ptr(co), _lib.ptr(mo), _lib.ptr(lw_out), C.byref(llk))))
    tc = report(f"(c) PPCA mixture iteration (ppca_mix_em_step, K = {nm})", t_c)
    td = report(f"(d) FA mixture iteration (ppca_famix_em_step, K = {nm})", t_d)
    # the host finalisation alone, on statistics of the right shape (S_cj = I, so that every row solve runs)
    slen = int(L.ppca_stats_len(d, k))
    kp = k * (k + 1) // 2
    st = rng.standard_normal((nm, slen))
    eye = np.array([1.0 if p_ == q_ else 0.0 for p_ in range(k) for q_ in range(p_ + 1)])
    st[:, d * k:d * k + d * kp] = np.tile(eye, d)
    st[:, 2 * d * k + d * kp + d:2 * d * k + d * kp + 2 * d] = 1.0  # totals
    sq = np.full((nm, d), 100.0)
    t0 = time.perf_counter()
    for _ in range(reps):
        _lib.check(L.ppca_famix_finalize_host(d, k, nm, _lib.ptr(fm._noise), _lib.ptr(fm._c), _lib.ptr(fm._mean), _lib.ptr(st), _lib.ptr(sq), None,
                                              None, _lib.ptr(no), _lib.ptr(co), _lib.ptr(mo)))
    tf = (time.perf_counter() - t0) * 1e3 / reps
    print(f"  (d) / (c) = {td / tc:.3f}   (d) - (c) = {td - tc:.3f} ms; the whitening {tw:.3f} ms, the sweep {tb:.3f} ms, "
          f"the host finalisation {tf:.3f} ms, the rest {td - tc - tw - tb - tf:.3f} ms")

if "--famix" in sys.argv:
    famix_legs(int(sys.argv[sys.argv.index("--famix") + 1]))
    sys.exit(0)

def moments_legs(reps=12):
    MFMA_TFLOPS = 47.9  # v_mfma_f64_16x16x4_f64 at two waves per SIMD, profiles/r04/mfma_peak.txt
    hip = C.CDLL(_lib.LIB_PATH)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []

    def series(fn):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts):
        med = float(np.median(ts))
        print(f"{name:44s} median {med:8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  max/median {ts.max()/med:5.3f}  "
              f"({reps} repetitions)", flush=True)
        return med

    center = ds.column_stats()[1]
    sums, counts, cross = np.empty((d, d)), np.empty((d, d)), np.empty((d, d))
    def moments(with_cross):
        _lib.check(L.ppca_dataset_pairwise_moments(ctx.handle, ds._h, _lib.ptr(center), _lib.ptr(sums), _lib.ptr(counts),
                                                   _lib.ptr(cross) if with_cross else None))
    out = C.c_void_p()
    _lib.check(L.ppca_model_alloc(ctx.handle, d, k, C.byref(out)))
    llk = C.c_double()
    def em():
        _lib.check(L.ppca_em_step(ctx.handle, ds._h, md.h, None, out, C.byref(llk)))
    dst = C.c_void_p()
    _lib.check(L.ppca_dataset_scale_columns(ctx.handle, ds._h, _lib.ptr(np.ones(d)), None, None, C.byref(dst), None, None))
    src_p, dst_p = L.ppca_dataset_device_x(ds._h), L.ppca_dataset_device_x(dst)
    def copy():
        assert hip.hipMemcpy(dst_p, src_p, C.c_size_t(8 * n * d), 3) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0
    t_em = report(f"PPCA iteration (ppca_em_step, k = {k})", series(em))
    t_cp = report("hipMemcpy device to device (N x d)", series(copy))
    t_s = report("pairwise moments: sums, counts", series(lambda: moments(False)))
    t_x = report("pairwise moments: sums, counts, cross", series(lambda: moments(True)))
    L.ppca_dataset_free(dst)
    L.ppca_model_free(out)
    sym = float(n) * d * (d + 1)  # flop of one symmetric matrix
    for name, t, flop in (("without cross", t_s, 2 * sym), ("with cross", t_x, 2 * sym + 2.0 * n * d * d)):
        print(f"  {name}: {t / t_em:6.2f} EM iterations, {t / t_cp:6.2f} copies of X, {flop / t / 1e9:6.2f} Tflop/s = "
              f"{flop / t / 1e9 / MFMA_TFLOPS:5.3f} of the measured fp64 MFMA rate ({MFMA_TFLOPS} Tflop/s)")
    print(f"  condition: without cross < 17 EM iterations: {t_s / t_em:.2f} -> {'met' if t_s < 17 * t_em else 'NOT met'}")

if "--moments" in sys.argv:
    moments_legs()
    sys.exit(0)

def kmeans_legs(nc, reps=12):
    from ppca_rs_amd.api import _kmeans_cluster_moments

    def series(fn, reps=reps):
        fn(); fn(); ctx.synchronize()  # warm-up: code objects, the block cache
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    def report(name, ts, nbytes=None):
        med = float(np.median(ts))
        rate = f"{nbytes/med/1e6:8.1f} GB/s" if nbytes else " " * 13
        print(f"{name:60s} median {med:9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}  {rate}  ({len(ts)} repetitions)", flush=True)
        return med

    rng = np.random.default_rng(5)
    nd_bytes = 8.0 * n * d
    _, mean, var = ds.column_stats()
    centers = np.ascontiguousarray(mean + np.sqrt(var) * rng.standard_normal((nc, d)))
    sums, inertia, reads = np.empty((nc, 2, d)), C.c_double(), C.c_int32()
    lab_buf = P.Dataset(np.zeros((n, 1)))  # n x 8 bytes on the device: the destination of the labels
    lab_dev = C.c_void_p(L.ppca_dataset_device_x(lab_buf._h))
    def step():
        _lib.check(L.ppca_dataset_kmeans_step(ctx.handle, ds._h, _lib.ptr(centers), None, nc, None, None, _lib.ptr(sums), C.byref(inertia),
                                              C.byref(reads)))
    def label():
        _lib.check(L.ppca_dataset_kmeans_step(ctx.handle, ds._h, _lib.ptr(centers), None, nc, lab_dev, None, None, C.byref(inertia),
                                              C.byref(reads)))
    # the composition the fused step replaces: labels, then the column sums of K one-hot weight vectors (device-resident)
    lab_host = np.zeros(n, dtype=np.int32)
    _lib.check(L.ppca_dataset_kmeans_step(ctx.handle, ds._h, _lib.ptr(centers), None, nc, _lib.ptr(lab_host), None, None, C.byref(inertia),
                                          C.byref(reads)))
    print(f"  rows per cluster under these centres: {np.bincount(lab_host, minlength=nc).tolist()}", flush=True)
    onehot = np.zeros((nc, n))
    onehot[lab_host, np.arange(n)] = 1.0  # the labels' own one-hot weights: what the composition would hand to the sweep
    del lab_host
    E = P.Dataset(onehot.reshape(-1, 1))
    del onehot
    e_dev = C.c_void_p(L.ppca_dataset_device_x(E._h))
    msums = np.empty((nc, 3, d))
    def multi():
        _lib.check(L.ppca_dataset_column_moments_multi(ctx.handle, ds._h, None, e_dev, nc, None, _lib.ptr(centers), _lib.ptr(msums)))
    def composition():
        label(); multi()
    one, ssums = np.ones(d), np.empty((3, d))
    def scale():
        _lib.check(L.ppca_dataset_scale_columns(ctx.handle, ds._h, _lib.ptr(one), _lib.ptr(mean), None, None, _lib.ptr(ssums), None))
    t_f, t_c, t_s = [], [], []
    for _ in range(2):  # the legs alternate, so that all see the same machine
        t_s.append(series(scale, reps // 2)); t_f.append(series(step, reps // 2)); t_c.append(series(composition, reps // 2))
    step()
    r_step = reads.value
    ts = report("(a) scale pass, sums only (one read of X: the floor)", np.concatenate(t_s), nd_bytes)
    tf = report(f"(b) Lloyd step, K = {nc} ({r_step} read{'s' if r_step != 1 else ''} of X)", np.concatenate(t_f), r_step * nd_bytes)
    tl = report(f"(c) labelling only, K = {nc} (labels to a device buffer)", series(label), nd_bytes)
    tc = report(f"(d) labelling + one-hot multi-component sweep, K = {nc}", np.concatenate(t_c), 2 * nd_bytes)
    print(f"  (b) / (a) = {tf / ts:.3f}   (c) / (a) = {tl / ts:.3f}   (b) / (d) = {tf / tc:.3f}   "
          f"({'the step is faster than the composition' if tf < tc else 'the step is NOT faster than the composition'})")
    del E
    kms = []
    def whole():
        kms.append(ds.kmeans(nc, seed=1))
    t_km = report(f"(e) Dataset.kmeans({nc}): seeding + Lloyd iterations + labels", series(whole, 3))
    km = kms[-1]
    print(f"  iterations run {km.n_iters_run}, converged {km.converged}, inertia {km.history[0]:.6g} -> {km.inertia:.6g}")
    t_mo = report(f"(f) the {nc} moment passes of from_kmeans", series(lambda: _kmeans_cluster_moments(ds, km), 3))
    comps = [P.PPCAModel(1.0, m.transform + 0.1 * rng.standard_normal((d, k)), m.mean) for _ in range(nc)]
    mix = P.PPCAMix(comps, np.full(nc, -np.log(nc)))
    devs, arr = mix._handles(ctx)
    outs = []
    for _ in range(nc):
        hh = C.c_void_p()
        _lib.check(L.ppca_model_alloc(ctx.handle, d, k, C.byref(hh)))
        outs.append(hh)
    oarr = (C.c_void_p * nc)(*outs)
    lw_out, llk = np.empty(nc), C.c_double()
    t_em = report(f"(g) PPCA mixture iteration (ppca_mix_em_step, K = {nc}, k = {k})",
                  series(lambda: _lib.check(L.ppca_mix_em_step(ctx.handle, ds._h, arr, _lib.ptr(mix._lw), nc, None, oarr, _lib.ptr(lw_out),
                                                               C.byref(llk)))))
    for hh in outs:
        L.ppca_model_free(hh)
    print(f"  the whole start: (e) + (f) = {t_km + t_mo:.3f} ms = {(t_km + t_mo) / t_em:.2f} mixture EM iterations "
          f"((e) {t_km / t_em:.2f}, (f) {t_mo / t_em:.2f}); one Lloyd step = {tf / t_em:.3f} iterations")

if "--kmeans" in sys.argv:
    kmeans_legs(int(sys.argv[sys.argv.index("--kmeans") + 1]))
    sys.exit(0)

def timed(name, fn, bytes_per_sample, reps=5):
    fn(); ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"{name:28s} {dt*1e3:9.2f} ms   {n/dt/1e6:8.1f} Msamples/s   {n*bytes_per_sample/dt/1e9:8.1f} GB/s algorithmic", flush=True)
    return out

tot = C.c_double()
timed("llk (total)", lambda: L.ppca_llk(ctx.handle, ds._h, md.h, C.byref(tot), None), 8 * d)
def recon(mode):
    o = C.c_void_p()
    _lib.check(L.ppca_reconstruct(ctx.handle, ds._h, md.h, mode, C.byref(o)))
    L.ppca_dataset_free(o)
timed("smooth (N x d out)", lambda: recon(0), 16 * d)
timed("extrapolate (N x d out)", lambda: recon(1), 16 * d)
def cdiag(mode):
    o = C.c_void_p()
    _lib.check(L.ppca_covariance_diagonal(ctx.handle, ds._h, md.h, mode, C.byref(o)))
    L.ppca_dataset_free(o)
timed("smoothed cov diagonal", lambda: cdiag(0), 16 * d)
def psample(mode):
    o = C.c_void_p()
    _lib.check(L.ppca_posterior_sample(ctx.handle, ds._h, md.h, mode, 7, 0, C.byref(o)))
    L.ppca_dataset_free(o)
timed("posterior sample", lambda: psample(0), 16 * d)
timed("posterior impute", lambda: psample(1), 16 * d)
def loo(full):
    mo, vo, tot = C.c_void_p(), C.c_void_p(), C.c_double()
    _lib.check(L.ppca_loo_predictive(ctx.handle, ds._h, md.h, C.byref(mo) if full else None, C.byref(vo) if full else None,
                                     C.byref(tot), None))
    if full:
        L.ppca_dataset_free(mo)
        L.ppca_dataset_free(vo)
timed("loo predictive (2 N x d out)", lambda: loo(True), 24 * d)
timed("loo llks only", lambda: loo(False), 8 * d)
nn = min(n, 1_000_000)
sub = ds._slice(0, nn)
st, cv = np.empty((nn, k)), np.empty((nn, k, k))
t0 = time.perf_counter(); _lib.check(L.ppca_infer(ctx.handle, sub._h, md.h, _lib.ptr(st), None)); t1 = time.perf_counter()
_lib.check(L.ppca_infer(ctx.handle, sub._h, md.h, _lib.ptr(st), _lib.ptr(cv))); t2 = time.perf_counter()
print(f"infer states only ({nn} rows, incl. D2H)      {1e3*(t1-t0):8.2f} ms")
print(f"infer states + covariances (incl. D2H {cv.nbytes/1e6:.0f} MB) {1e3*(t2-t1):8.2f} ms")
del st, cv
nh = min(nn, max(1000, (1 << 32) // (8 * k * k * 3)))  # the host sampler holds about three N x k x k arrays: 4 GB at most
hs = ds._slice(0, nh)
t3 = time.perf_counter(); m.infer(hs).posterior_sampler().sample(seed=7); t4 = time.perf_counter()
o = C.c_void_p()
_lib.check(L.ppca_posterior_sample(ctx.handle, hs._h, md.h, 0, 7, 0, C.byref(o))); t5 = time.perf_counter()
L.ppca_dataset_free(o)
print(f"host posterior sampler ({nh} rows: infer + numpy + upload) {1e3*(t4-t3):8.2f} ms   device posterior sample, same rows {1e3*(t5-t4):8.2f} ms")
if "--mix" in sys.argv:  # the mixture's leave-one-out predictive over nm components of state size k (perturbed copies of m)
    nm = int(sys.argv[sys.argv.index("--mix") + 1])
    rng = np.random.default_rng(4)
    mix = P.PPCAMix([P.PPCAModel(m.isotropic_noise * (1 + 0.1 * c_), m.transform + 0.1 * rng.standard_normal((d, k)), m.mean)
                     for c_ in range(nm)], np.full(nm, -np.log(nm)))
    devs, arr = mix._handles(ctx)
    def mloo(full):
        mo, vo, tot = C.c_void_p(), C.c_void_p(), C.c_double()
        _lib.check(L.ppca_mix_loo_predictive(ctx.handle, ds._h, arr, _lib.ptr(mix._lw), nm, C.byref(mo) if full else None,
                                             C.byref(vo) if full else None, C.byref(tot), None))
        if full:
            L.ppca_dataset_free(mo)
            L.ppca_dataset_free(vo)
    def mrecon(mode):
        o = C.c_void_p()
        _lib.check(L.ppca_mix_reconstruct(ctx.handle, ds._h, arr, _lib.ptr(mix._lw), nm, mode, C.byref(o)))
        L.ppca_dataset_free(o)
    timed(f"mix({nm}) extrap cov diagonal", lambda: mrecon(3), 16 * d, reps=2)
    timed(f"mix({nm}) loo predictive", lambda: mloo(True), 24 * d, reps=2)
    timed(f"mix({nm}) loo llks only", lambda: mloo(False), 8 * d, reps=2)
