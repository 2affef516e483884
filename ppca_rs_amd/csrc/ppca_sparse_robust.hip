// ppca_sparse_robust.hip -- Student-t PPCA on row-compressed data (ppca_t_sparse_estep, ppca_t_sparse_em_step; DESIGN.md section
// 4.28).  Storage, the values view and shared scaffolding: ppca_sparse.hpp.  The model and its quantities are those of ppca_robust.hip
// (DESIGN.md section 4.15); the row's posterior mean z and Gaussian log-density come from sparse_row_kernel<K> (sp_rows_of_block).
// sparse_t_row_kernel<K>  the CSR orientation, the groups and bins of sparse_row_kernel (W = 4 / 16 / 64 by row length).  Lane s takes
//     the row's entries s, s + W, ... in order, forms x~ = val - mean[col], r = x~ - c_col . z and adds r^2; one butterfly adds the
//     lanes.  Then delta, u, ell as ppca_robust.hip forms them, and on a second walk over the same entries the scaled values
//     out_val = fl(fl(sqrt u) fl(x~)).  Outputs, all nullable: u, delta, ell per row, the scaled CSR values, the record
//     [w u z (K) | w u | fl(sqrt u)] and the row's scalar terms [w | w ell | w (g[m] + ln u - u) | non-empty].  A row's outputs depend
//     on its entry list alone.
// sparse_t_scal_kernel    sparse_scal_kernel for the four scalar terms: 1024 rows per workgroup in a fixed tree, padded to the eight
//     slots of launch_reduce_partials.
// sparse_t_col_kernel<K>  the index orientation, the work items, groups and runs of sparse_col_kernel.  Lane o of an item's group owns
//     output o of [V_j (K) | A_j | T_j | sq_j] and adds the item's entries in ascending row, each entry gathering its row's record;
//     with a view, out_tval = fl(rec.sqrt u * fl(tval - mean_j)): the operands of the CSR copy, hence its bits.  A whole column adds
//     its sum (blocks in stream order); a run writes its partial and sparse_t_fix_kernel adds a column's runs in run order.  No float
//     atomics.
// The step scales into a view, runs sp_accumulate on it under PPCAModel(sigma, C, 0) and hands statistics and sums to
// ppca_t_finalize_host.
#include <cmath>
#include <cstring>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

constexpr int SP_T_NSCAL = 4;  // per-row scalar terms: w | w ell | w (g[m] + ln u - u) | non-empty

struct SpTRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const double *w;      // nullable, indexed by global row
    const int32_t *rows;  // a bin of the block's rows, local to the block
    int64_t nrows, row0;
    int W, d;
    const double *model;
    const double *lg, *g;          // the tables of ppca_t_tables_host, entries 0 .. the longest row
    const double *llks, *states;   // the Gaussian row pass, indexed by the row within the block
    double nu;
    double *u, *maha, *ell;  // nullable, indexed by global row
    double *out_val;         // nullable, CSR order
    double *rec, *rscal;     // nullable, indexed by the row within the block
};

template <int K>
__global__ __launch_bounds__(256) void sparse_t_row_kernel(SpTRowArgs a) {
    constexpr int NR = K + 2;
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1], nu = a.nu;
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        double z[K], zz = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            z[t] = live ? a.states[lr * K + t] : 0.0;
            zz = fma(z[t], z[t], zz);
        }
        double ss = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            const double xt = __dsub_rn(a.val[e], mu[j]);
            const double *cj = C + (int64_t)j * K;
            double dot = 0.0;
#pragma unroll
            for (int t = 0; t < K; ++t) dot = fma(cj[t], z[t], dot);
            const double res = xt - dot;
            ss = fma(res, res, ss);
        }
        // the group's lanes, one butterfly: the same tree for every row of the bin, the same sum on every lane
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
            if (o < W) ss += __shfl_xor(ss, o, 64);
        const int m = (int)(e1 - e0);
        const double md = (double)m;
        const double delta = m > 0 ? fma(s2, zz, ss) / s2 : 0.0;
        const double ub = m > 0 ? (nu + md) / (nu + delta) : 1.0;
        const double su = sqrt(ub);
        if (a.out_val) {  // (uniform) the same entries again, now that the row's weight is known
            for (int64_t e = e0 + sub; e < e1; e += W) a.out_val[e] = __dmul_rn(su, __dsub_rn(a.val[e], mu[a.col[e]]));
        }
        if (live && sub == 0) {
            const double lk = a.llks[lr];
            const double logdet = -2.0 * lk - md * LN_2PI - delta;
            const double el = m > 0 ? a.lg[m] - 0.5 * logdet - 0.5 * (nu + md) * log1p(delta / nu) : 0.0;
            const double w = a.w ? a.w[r] : 1.0;
            if (a.u) a.u[r] = ub;
            if (a.maha) a.maha[r] = delta;
            if (a.ell) a.ell[r] = el;
            if (a.rec) {
                double *rec = a.rec + lr * NR;
                const double wu = w * ub;
#pragma unroll
                for (int t = 0; t < K; ++t) rec[t] = wu * z[t];
                rec[K] = wu;
                rec[K + 1] = su;
            }
            if (a.rscal) {
                double *sc = a.rscal + lr * SP_T_NSCAL;
                sc[0] = w;
                sc[1] = w * el;
                sc[2] = w * (a.g[m] + log(ub) - ub);  // (an empty row: g[0] - 1)
                sc[3] = m > 0 ? 1.0 : 0.0;
            }
        }
    }
}

// part[blockIdx][8] = the sums of the scalar terms of rows [1024 blockIdx, ...), slots 4 .. 7 zero: thread t adds rows t, t + 256, ..
// in order, then a fixed tree over the threads (sparse_scal_kernel's)
__global__ __launch_bounds__(256) void sparse_t_scal_kernel(const double *rscal, int64_t rows, double *part) {
    __shared__ double red[256][SP_T_NSCAL];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SP_SCAL_ROWS;
    double s[SP_T_NSCAL] = {0, 0, 0, 0};
    for (int i = 0; i < SP_SCAL_ROWS / 256; ++i) {
        const int64_t r = r0 + tid + 256 * i;
        if (r < rows) {
#pragma unroll
            for (int q = 0; q < SP_T_NSCAL; ++q) s[q] += rscal[r * SP_T_NSCAL + q];
        }
    }
#pragma unroll
    for (int q = 0; q < SP_T_NSCAL; ++q) red[tid][q] = s[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < SP_T_NSCAL; ++q) red[tid][q] += red[tid + o][q];
        }
        __syncthreads();
    }
    if (tid < 8) part[(int64_t)blockIdx.x * 8 + tid] = tid < SP_T_NSCAL ? red[0][tid] : 0.0;
}

template <int K>
struct SpTColCfg {
    static constexpr int NR = K + 2, NO = K + 3;
    static constexpr int GW = NO <= 8 ? 8 : NO <= 16 ? 16 : 32;
};
// where output o of column j lives in [V (d x k) | A | T | sq]
__device__ __forceinline__ int64_t sp_t_sum_index(int o, int j, int d, int k) {
    return o < k ? (int64_t)j * k + o : (int64_t)d * k + (int64_t)(o - k) * d + j;
}

struct SpTColArgs {
    const SpItem *items;
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *rec;  // the block's records
    const double *model;
    int d;
    double *out_tval;  // nullable, inverted-index order
    double *sums;      // nullable, (k + 3) d
    double *runpart;
};

template <int K>
__global__ __launch_bounds__(256) void sparse_t_col_kernel(SpTColArgs a) {
    using Cf = SpTColCfg<K>;
    constexpr int GW = Cf::GW, NR = Cf::NR, NO = Cf::NO, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1), gbase = lane & ~(GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double *mu = a.model + MODEL_HDR + (int64_t)a.d * K;
    const int slot = sub < K ? sub : K;  // the record element behind output `sub`: w u z_o, else w u
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double muj = mu[it.col];
        double acc = 0.0;
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group)
            const bool mine = t + sub < it.len;
            const int li = mine ? a.trow[it.start + t + sub] : 0;
            const double xv = mine ? __dsub_rn(a.tval[it.start + t + sub], muj) : 0.0;
            if (a.out_tval && mine) a.out_tval[it.start + t + sub] = __dmul_rn(a.rec[(int64_t)li * NR + K + 1], xv);
            if (!a.sums) continue;  // (uniform)
            const int nb = it.len - t < GW ? it.len - t : GW;
            for (int q = 0; q < nb; q += 4) {  // the entries in ascending row, four record gathers in flight
                double f[4], v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int src = gbase + ((q + u) & (GW - 1));
                    const int i = __shfl(li, src, 64);
                    const double x = __shfl(xv, src, 64);
                    const bool ok = q + u < nb && sub < NO;  // (past the end: exact zeros, which change no sum)
                    v[u] = ok ? a.rec[(int64_t)i * NR + slot] : 0.0;
                    f[u] = sub == K ? x : sub == K + 2 ? __dmul_rn(x, x) : 1.0;  // V, T: the record itself; A: times x~; sq: times x~^2
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = fma(v[u], f[u], acc);
            }
        }
        if (live && a.sums && sub < NO) {
            if (it.dest < 0) {
                double *dst = a.sums + sp_t_sum_index(sub, it.col, a.d, K);
                *dst += acc;
            } else {
                a.runpart[it.dest * NO + sub] = acc;
            }
        }
    }
}

// sums of a long column += its runs' partials, added in run order
__global__ __launch_bounds__(256) void sparse_t_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, int k, double *sums) {
    const int no = k + 3;
    for (int64_t c = blockIdx.x; c < n_long; c += gridDim.x) {
        const SpLong lc = longs[c];
        for (int o = threadIdx.x; o < no; o += blockDim.x) {
            double s = 0.0;
            for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * no + o];
            sums[sp_t_sum_index(o, lc.col, d, k)] += s;
        }
    }
}

}  // namespace ppca_sp

namespace {

template <int K>
hipError_t t_row_t(const SpTRowArgs &a, int grid, hipStream_t s) { return sp_launch(sparse_t_row_kernel<K>, grid, s, a); }
template <int K>
hipError_t t_col_t(const SpTColArgs &a, int n_cu, hipStream_t s) {
    return sp_launch(sparse_t_col_kernel<K>, sp_grid(a.n_items, 4 * (64 / SpTColCfg<K>::GW), n_cu, 8), s, a);
}
hipError_t launch_t_row(int k, const SpTRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, t_row_t, a, grid, s); }
hipError_t launch_t_col(int k, const SpTColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, t_col_t, a, n_cu, s); }

// the longest row any dataset of this shape can hold: the tables are built to there
int64_t sp_t_table_len(const SpCore &c) { return std::min<int64_t>(c.d, c.nnz) + 1; }

// What an E-step keeps alive until the caller's synchronisation: the host side of its asynchronous upload and its device scratch.
struct SpTSweep {
    std::vector<double> tabs;  // [lg | g] as uploaded
    BufRef tabs_dev, llks, states, rec, rscal, spart, runpart, sums, scal;
    double *sums_dev() const { return sums ? dptr<double>(sums) : nullptr; }
};

// Enqueues the E-step of sp under (model, dof): view (nullable) gets buffers of its own for sqrt(u) (x - mean) in both orientations, on
// sp's core and weights; want_sums: the (k + 3) d column sums into sw.sums; u, maha, ell (nullable): n doubles each on the device.  The
// four scalars go to sw.scal (8 doubles).  The column kernel runs when a view or the sums are wanted.  No wait.
int sp_t_sweep(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, double dof, ppca_sparse *view, bool want_sums, double *u,
               double *maha, double *ell, SpTSweep &sw) {
    const SpCore &c = *sp->core;
    const int k = model->k;
    const int64_t tl = sp_t_table_len(c), rows = std::max<int64_t>(c.max_rows, 1);
    sw.tabs.resize((size_t)2 * tl);
    if (int rc = ppca_t_tables_host((int32_t)(tl - 1), dof, sw.tabs.data(), sw.tabs.data() + tl)) return rc;
    if (int rc = sp_upload(ctx, sw.tabs.data(), sizeof(double) * sw.tabs.size(), &sw.tabs_dev)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)rows, &sw.llks)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)rows * k, &sw.states)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)rows * SP_T_NSCAL, &sw.rscal)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8 * (size_t)((rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS), &sw.spart)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8, &sw.scal)) return rc;
    HIP_TRY(hipMemsetAsync(sw.scal->p, 0, sizeof(double) * 8, ctx->stream));
    double *ov = nullptr, *otv = nullptr;
    if (view) {
        view->ctx = sp->ctx;
        view->core = sp->core;
        view->wbuf = sp->wbuf;
        view->w = sp->w;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.nnz, 1), &view->vbuf)) return rc;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.nnz, 1), &view->tvbuf)) return rc;
        ov = dptr<double>(view->vbuf);
        otv = dptr<double>(view->tvbuf);
    }
    const bool cols = otv || want_sums;
    if (cols)
        if (int rc = dev_alloc(sizeof(double) * (size_t)rows * (k + 2), &sw.rec)) return rc;
    if (want_sums) {
        if (int rc = dev_alloc(sizeof(double) * (size_t)(k + 3) * c.d, &sw.sums)) return rc;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * (k + 3), &sw.runpart)) return rc;
        HIP_TRY(hipMemsetAsync(sw.sums->p, 0, sizeof(double) * (size_t)(k + 3) * c.d, ctx->stream));
    }
    double *runpart = sw.runpart ? dptr<double>(sw.runpart) : nullptr;
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_rows_of_block(ctx, sp, b, model, dptr<double>(sw.llks), dptr<double>(sw.states), nullptr, nullptr, nullptr)) return rc;
        SpTRowArgs ra{};
        ra.w = sp->w;
        ra.d = c.d;
        ra.model = model->p();
        ra.lg = dptr<const double>(sw.tabs_dev);
        ra.g = ra.lg + tl;
        ra.llks = dptr<const double>(sw.llks);
        ra.states = dptr<const double>(sw.states);
        ra.nu = dof;
        ra.u = u;
        ra.maha = maha;
        ra.ell = ell;
        ra.out_val = ov;
        ra.rec = cols ? dptr<double>(sw.rec) : nullptr;
        ra.rscal = dptr<double>(sw.rscal);
        const auto row = [&](const SpTRowArgs &a, int grid) { return launch_t_row(k, a, grid, ctx->stream); };
        if (int rc = sp_for_bins(ctx, sp, b, ra, row)) return rc;
        const int parts = (int)((b.rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS);
        HIP_TRY(sp_launch(sparse_t_scal_kernel, parts, ctx->stream, dptr<const double>(sw.rscal), b.rows, dptr<double>(sw.spart)));
        HIP_TRY(launch_reduce_partials(dptr<double>(sw.spart), parts, 8, dptr<double>(sw.scal), ctx->stream, 1));
        if (!cols) continue;
        SpTColArgs ca{};
        ca.rec = dptr<const double>(sw.rec);
        ca.model = model->p();
        ca.out_tval = otv;
        ca.sums = sw.sums_dev();
        const auto item = [&](const SpTColArgs &a) { return launch_t_col(k, a, ctx->n_cu, ctx->stream); };
        const auto fix = [&] {  // one workgroup per long column
            if (!want_sums) return hipSuccess;
            return sp_launch(sparse_t_fix_kernel, sp_grid(b.n_long, 1, ctx->n_cu, 8), ctx->stream, b.longs(), b.n_long, (const double *)runpart, c.d, k,
                             sw.sums_dev());
        };
        if (int rc = sp_col_pass(sp, b, runpart, ca, item, fix)) return rc;
    }
    return PPCA_OK;
}

int sp_t_check_dof(double dof) {
    return dof > 0.0 && std::isfinite(dof) ? PPCA_OK : fail(PPCA_ERR_INVALID, "dof must be a positive finite number");
}
int sp_t_check_k(int k) {
    if (k >= 1 && k <= SP_MAX_K) return PPCA_OK;
    return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported by the Student-t model on sparse data: the kernels cover 1 <= k <= %d", k,
                SP_MAX_K);
}

// the device image of a model, [sigma, sigma^2, ln sigma, 0 | C (d x k) | mean] (mean == nullptr: zeros)
std::vector<double> sp_t_model_image(double sigma, const double *C, const double *mean, int d, int k) {
    std::vector<double> h((size_t)model_len(d, k), 0.0);
    h[0] = sigma;
    h[1] = sigma * sigma;
    h[2] = std::log(sigma);
    std::memcpy(h.data() + MODEL_HDR, C, sizeof(double) * (size_t)d * k);
    if (mean) std::memcpy(h.data() + MODEL_HDR + (size_t)d * k, mean, sizeof(double) * d);
    return h;
}

typedef std::unique_ptr<ppca_model, int (*)(ppca_model *)> SpTModel;
// a model of the context whose image is uploaded without a wait: h is read until the stream's next synchronisation
int sp_t_model(ppca_ctx *ctx, int d, int k, const std::vector<double> &h, SpTModel &out) {
    ppca_model *raw = nullptr;
    if (int rc = ppca_model_alloc(ctx, d, k, &raw)) return rc;
    out.reset(raw);
    touch(raw);
    HIP_TRY(hipMemcpyAsync(raw->p(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
    return PPCA_OK;
}

}  // namespace

extern "C" int ppca_t_sparse_estep(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double dof, ppca_sparse **scaled_out,
                                   double *col_sums_host, double *u_host, double *maha_host, double *llks_host, double *scalars_host) {
    if (!ctx || !sp || !model) return fail(PPCA_ERR_INVALID, "null argument");
    if (!scaled_out && !col_sums_host && !u_host && !maha_host && !llks_host && !scalars_host)
        return fail(PPCA_ERR_INVALID, "no output requested");
    const SpCore &c = *sp->core;
    if (c.d != model->d) return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", c.d, model->d);
    if (sp->ctx->device != model->ctx->device || sp->ctx->device != ctx->device)
        return fail(PPCA_ERR_INVALID, "dataset, model and context live on different devices");
    if (int rc = sp_t_check_dof(dof)) return rc;
    if (int rc = sp_t_check_k(model->k_user())) return rc;
    USE_CTX(ctx);
    const int k = model->k;
    const size_t n = (size_t)c.n, ncs = (size_t)(k + 3) * c.d;
    std::unique_ptr<ppca_sparse> view(scaled_out ? new ppca_sparse() : nullptr);
    SpTSweep sw;  // (its table is read by the upload: alive until the synchronisation below)
    BufRef ub, mb, lb;
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = PPCA_OK;
    if (!rc && u_host && n) rc = dev_alloc(sizeof(double) * n, &ub);
    if (!rc && maha_host && n) rc = dev_alloc(sizeof(double) * n, &mb);
    if (!rc && llks_host && n) rc = dev_alloc(sizeof(double) * n, &lb);
    if (!rc)
        rc = sp_t_sweep(ctx, sp, model, dof, view.get(), col_sums_host != nullptr, ub ? dptr<double>(ub) : nullptr, mb ? dptr<double>(mb) : nullptr,
                        lb ? dptr<double>(lb) : nullptr, sw);
    const auto down = [&](void *dst, const BufRef &src, size_t bytes) {
        if (!rc && src && hipMemcpyAsync(dst, src->p, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            rc = fail(PPCA_ERR_HIP, "download failed");
    };
    down(u_host, ub, sizeof(double) * n);
    down(maha_host, mb, sizeof(double) * n);
    down(llks_host, lb, sizeof(double) * n);
    if (col_sums_host) down(col_sums_host, sw.sums, sizeof(double) * ncs);
    down(h, sw.scal, sizeof(h));
    if ((rc = sp_finish(ctx, rc, "t E-step"))) return rc;  // (the upload reads sw.tabs)
    if (scalars_host) std::memcpy(scalars_host, h, sizeof(double) * 4);
    if (scaled_out) *scaled_out = view.release();
    return PPCA_OK;
}

extern "C" int ppca_t_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, int32_t d, int32_t k, double sigma, const double *transform,
                                     const double *mean, double dof, double *sigma_out, double *transform_out, double *mean_out,
                                     double *llk_in, double *q_out) {
    if (!ctx || !sp || !transform || !mean || !sigma_out || !transform_out || !mean_out) return fail(PPCA_ERR_INVALID, "null argument");
    if (d < 1 || k < 0) return fail(PPCA_ERR_INVALID, "invalid shape d=%d k=%d", d, k);
    const SpCore &c = *sp->core;
    if (c.d != d) return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", c.d, d);
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(PPCA_ERR_INVALID, "sigma is not a positive finite number");
    if (int rc = sp_t_check_dof(dof)) return rc;
    if (int rc = sp_t_check_k(k)) return rc;
    if (c.n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    USE_CTX(ctx);
    // the model (sigma, C, mean) of the E-step and (sigma, C, 0) of the EM pass on the centred, scaled view: uploaded without a wait
    // (hm, hm0 and the sweep's table are read until the synchronisation below)
    const std::vector<double> hm = sp_t_model_image(sigma, transform, mean, d, k), hm0 = sp_t_model_image(sigma, transform, nullptr, d, k);
    const StatsLayout L(d, k);
    std::vector<double> hs((size_t)L.len), sums((size_t)(k + 3) * d);
    double sc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SpTModel m(nullptr, ppca_model_free), m0(nullptr, ppca_model_free);
    SpTSweep sw;
    ppca_sparse view;  // (its two buffers go back to the context's block cache when it leaves scope)
    double *stats = nullptr;
    int rc = sp_t_model(ctx, d, k, hm, m);
    if (!rc) rc = sp_t_model(ctx, d, k, hm0, m0);
    if (!rc) rc = ensure(ctx->stats, ctx->stats_cap, sizeof(double) * (size_t)L.len);
    if (!rc) {
        stats = dptr<double>(ctx->stats);
        ctx->stats_llk_at = -1;  // (the llk in the buffer is the scaled view's Gaussian one: ppca_em_last_llk does not apply)
        rc = sp_t_sweep(ctx, sp, m.get(), dof, &view, true, nullptr, nullptr, nullptr, sw);
    }
    if (!rc) rc = sp_accumulate(ctx, &view, m0.get(), stats);
    if (!rc && hipMemcpyAsync(sums.data(), sw.sums->p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(sc, sw.scal->p, sizeof(sc), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(hs.data(), stats, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if ((rc = sp_finish(ctx, rc, "t step"))) return rc;  // the one wait (the uploads read hm, hm0 and the table)
    if (int frc = ppca_t_finalize_host(d, k, sigma, transform, mean, hs.data(), sums.data(), sigma_out, transform_out, mean_out)) return frc;
    if (llk_in) *llk_in = sc[1];
    if (q_out) *q_out = sc[0] > 0.0 ? sc[2] / sc[0] : 0.0;
    return PPCA_OK;
}
