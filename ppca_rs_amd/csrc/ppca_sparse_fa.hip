// ppca_sparse_fa.hip -- column rescaling and factor analysis on row-compressed data (ppca_scale_columns_sparse,
// ppca_fa_sparse_em_step).  Storage, the values view and shared scaffolding: ppca_sparse.hpp.
// sparse_scale_row_kernel  the CSR orientation, sparse_held_row_kernel's groups and bins: out_val = val * a[col] (one fp64 multiply)
//     and, optionally, the row's sum of l[col], lane s adding the entries s, s + W, ... in order, one butterfly.
// sparse_scale_col_kernel  the index orientation, sparse_held_col_kernel's items, 16-lane groups and runs: out_tval = tval * a_j (the
//     same multiply, the same bits) and, optionally, [sum w | sum w (x a_j - b_j) | sum w (x a_j - b_j)^2] per column: chunks of 16 by
//     butterfly, chunks in order, sparse_colsum_fix_kernel<3> adds a column's runs in run order.  No float atomics.
// The FA step whitens into a view, runs sp_accumulate on it under PPCAModel(1, C / s, mean / s) and hands the statistics to
// ppca_fa_finalize_host.
#include <cmath>
#include <cstring>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

// ---- the column rescaling behind factor analysis on row-compressed data
struct SpScaleRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const int32_t *rows;  // a bin of the block's rows, local to the block
    int64_t nrows, row0;
    int W;
    const double *a, *l;  // per column (l read only with rowsum)
    double *out_val;      // nullable, CSR order
    double *rowsum;       // nullable, indexed by global row
};

// The CSR orientation: the groups and bins of sparse_held_row_kernel.  Lane s of a row's group takes the entries s, s + W, ...: each
// gets out_val = val * a[col] (one fp64 multiply) and the lane adds l[col] in that order; one butterfly adds the lanes.  The gather of
// a[col] / l[col] is per entry (the columns of a row are scattered): 8 d bytes each, which stay in L2.
__global__ __launch_bounds__(256) void sparse_scale_row_kernel(SpScaleRowArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        double lsum = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            if (a.out_val) a.out_val[e] = __dmul_rn(a.val[e], a.a[j]);
            if (a.rowsum) lsum += a.l[j];
        }
        if (a.rowsum) {  // (uniform) the group's lanes, one butterfly: the same tree for every row of the bin
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
                if (o < W) lsum += __shfl_xor(lsum, o, 64);
            if (live && sub == 0) a.rowsum[r] = lsum;
        }
    }
}

constexpr int SP_SCALE_GW = 16;  // lanes of an item's group in sparse_scale_col_kernel
constexpr int SP_SCALE_NO = 3;   // sums per column: w | w (x a - b) | w (x a - b)^2

struct SpScaleColArgs {
    const SpItem *items;  // the work items of the inverted index
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *w;  // row weights (nullable), indexed by global row
    int64_t row0;
    const double *a, *b;  // per column
    int d;
    double *out_tval;  // nullable, inverted-index order
    double *colsum;    // nullable, 3 x d
    double *runpart;
};

// The index orientation: the work items, 16-lane groups and run partials of sparse_held_col_kernel.  Lane s takes the entries s,
// s + 16, ... of the item (ascending row): out_tval = tval * a_j, the multiply of the row kernel on the same operands, and
// [w | w r | w r^2] with r = x a_j - b_j.  Each chunk of 16 entries is added by one butterfly and the chunks in order.  A whole column
// adds into the 3 x d sums (blocks in stream order); a run writes a partial and sparse_colsum_fix_kernel<3> adds a column's runs in run
// order.  a_j and b_j are uniform over the group.  No float atomics.
__global__ __launch_bounds__(256) void sparse_scale_col_kernel(SpScaleColArgs a) {
    constexpr int GW = SP_SCALE_GW, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double aj = a.a[it.col], bj = a.b[it.col];
        double acc[SP_SCALE_NO] = {0.0, 0.0, 0.0};
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group) one chunk of GW entries, ascending row
            double p[SP_SCALE_NO] = {0.0, 0.0, 0.0};  // (past the end: exact zeros, which change no sum)
            if (t + sub < it.len) {
                const int64_t at = it.start + t + sub;
                const double y = __dmul_rn(a.tval[at], aj);
                if (a.out_tval) a.out_tval[at] = y;
                if (a.colsum) {
                    const double w = a.w ? a.w[a.row0 + a.trow[at]] : 1.0;
                    const double r = y - bj;
                    p[0] = w;
                    p[1] = w * r;
                    p[2] = w * __dmul_rn(r, r);
                }
            }
            if (a.colsum) {  // (uniform)
#pragma unroll
                for (int o = 1; o < GW; o <<= 1)
#pragma unroll
                    for (int q = 0; q < SP_SCALE_NO; ++q) p[q] += __shfl_xor(p[q], o, 64);
#pragma unroll
                for (int q = 0; q < SP_SCALE_NO; ++q) acc[q] += p[q];
            }
        }
        if (a.colsum && live && sub < SP_SCALE_NO) {
            const double s = sub == 0 ? acc[0] : sub == 1 ? acc[1] : acc[2];
            if (it.dest < 0)
                a.colsum[(int64_t)sub * a.d + it.col] += s;
            else
                a.runpart[it.dest * SP_SCALE_NO + sub] = s;
        }
    }
}

}  // namespace ppca_sp

namespace {

// Enqueues the rescaling of sp under the device vectors abl = [a | b | l] (3 d): view (nullable) gets buffers of its own for
// val * a[col] in both orientations, on sp's core and weights; colsum (nullable, 3 x d, device) and rowsum (nullable, n, device) the
// sums.  The row kernel runs when a view or the row sums are wanted, the column kernel when a view or the column sums are.  No wait.
int sp_scale(ppca_ctx *ctx, const ppca_sparse *sp, const double *abl, ppca_sparse *view, double *colsum, double *rowsum) {
    const SpCore &c = *sp->core;
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
    BufRef runbuf;
    double *runpart = nullptr;
    if (colsum) {
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * SP_SCALE_NO, &runbuf)) return rc;
        runpart = dptr<double>(runbuf);
        HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(double) * (size_t)SP_SCALE_NO * c.d, ctx->stream));
    }
    for (const SpBlock &b : c.blocks) {
        if (ov || rowsum) {
            SpScaleRowArgs ra{};
            ra.a = abl;
            ra.l = abl + (size_t)2 * c.d;
            ra.out_val = ov;
            ra.rowsum = rowsum;
            const auto row = [&](const SpScaleRowArgs &a, int grid) { return sp_launch(sparse_scale_row_kernel, grid, ctx->stream, a); };
            if (int rc = sp_for_bins(ctx, sp, b, ra, row)) return rc;
        }
        if (!otv && !colsum) continue;
        SpScaleColArgs ca{};
        ca.w = sp->w;
        ca.row0 = b.row0;
        ca.a = abl;
        ca.b = abl + c.d;
        ca.out_tval = otv;
        ca.colsum = colsum;
        const auto item = [&](const SpScaleColArgs &a) {
            return sp_launch(sparse_scale_col_kernel, sp_grid(a.n_items, 4 * (64 / SP_SCALE_GW), ctx->n_cu, 8), ctx->stream, a);
        };
        const auto fix = [&] { return colsum ? sp_colsum_fix<SP_SCALE_NO>(ctx, b, runpart, c.d, colsum) : hipSuccess; };
        if (int rc = sp_col_pass(sp, b, runpart, ca, item, fix)) return rc;
    }
    return PPCA_OK;
}

// [a | b | l] (b, l nullable = 0) on the device; h: the caller's staging vector, read until the stream's next synchronisation
int sp_upload_abl(ppca_ctx *ctx, int d, const double *a, const double *b, const double *l, std::vector<double> &h, BufRef *out) {
    h.assign((size_t)3 * d, 0.0);
    std::memcpy(h.data(), a, sizeof(double) * d);
    if (b) std::memcpy(h.data() + d, b, sizeof(double) * d);
    if (l) std::memcpy(h.data() + (size_t)2 * d, l, sizeof(double) * d);
    return sp_upload(ctx, h.data(), sizeof(double) * h.size(), out);
}

int sp_check_finite(const double *v, int d, const char *name) {
    if (v)
        for (int j = 0; j < d; ++j)
            if (!std::isfinite(v[j])) return fail(PPCA_ERR_INVALID, "%s[%d] is not a finite number", name, j);
    return PPCA_OK;
}

}  // namespace

extern "C" int ppca_scale_columns_sparse(ppca_ctx *ctx, ppca_sparse *sp, const double *a_host, const double *b_host, const double *l_host,
                                         ppca_sparse **out, double *col_sums_host, double *row_sums_host) {
    if (!ctx || !sp || !a_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (!out && !col_sums_host && !row_sums_host) return fail(PPCA_ERR_INVALID, "no output requested");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    const SpCore &c = *sp->core;
    if (int rc = sp_check_finite(a_host, c.d, "a")) return rc;
    if (int rc = sp_check_finite(b_host, c.d, "b")) return rc;
    if (int rc = sp_check_finite(l_host, c.d, "l")) return rc;
    USE_CTX(ctx);
    std::unique_ptr<ppca_sparse> view(out ? new ppca_sparse() : nullptr);
    std::vector<double> h;  // (read by the upload: alive until the synchronisation below)
    BufRef abl, cs, rs;
    int rc = sp_upload_abl(ctx, c.d, a_host, b_host, l_host, h, &abl);
    if (!rc && col_sums_host) rc = dev_alloc(sizeof(double) * (size_t)SP_SCALE_NO * c.d, &cs);
    if (!rc && row_sums_host && c.n > 0) rc = dev_alloc(sizeof(double) * (size_t)c.n, &rs);
    if (!rc)
        rc = sp_scale(ctx, sp, dptr<const double>(abl), view.get(), cs ? dptr<double>(cs) : nullptr, rs ? dptr<double>(rs) : nullptr);
    if (!rc && cs && hipMemcpyAsync(col_sums_host, cs->p, sizeof(double) * (size_t)SP_SCALE_NO * c.d, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && rs && hipMemcpyAsync(row_sums_host, rs->p, sizeof(double) * (size_t)c.n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if ((rc = sp_finish(ctx, rc, "scale pass"))) return rc;  // (the upload reads `h`)
    if (out) *out = view.release();
    return PPCA_OK;
}

extern "C" int ppca_fa_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, int32_t d, int32_t k, const double *noise, const double *transform,
                                      const double *mean, const double *min_noise, double *noise_out, double *transform_out,
                                      double *mean_out, double *llk_in) {
    if (!ctx || !sp || !noise || !mean || !noise_out || !mean_out || d < 1 || k < 0 || (k > 0 && (!transform || !transform_out)))
        return fail(PPCA_ERR_INVALID, "null argument");
    const SpCore &c = *sp->core;
    if (c.d != d) return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", c.d, d);
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    if (k > SP_MAX_K)
        return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported on sparse data: the kernels cover k <= %d", k, SP_MAX_K);
    if (c.n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    for (int j = 0; j < d; ++j)
        if (!(noise[j] > 0.0) || !std::isfinite(noise[j])) return fail(PPCA_ERR_INVALID, "noise[%d] is not a positive finite number", j);
    USE_CTX(ctx);
    // the whitened model PPCAModel(1, A, mean~) and the whitening vectors a = 1 / s, b = mean / s, as ppca_fa_em_step forms them
    std::vector<double> inv((size_t)d), mw((size_t)d), A((size_t)d * k), sums((size_t)SP_SCALE_NO * d);
    for (int j = 0; j < d; ++j) {
        inv[j] = 1.0 / noise[j];
        mw[j] = mean[j] / noise[j];
        for (int b = 0; b < k; ++b) A[(int64_t)j * k + b] = transform[(int64_t)j * k + b] / noise[j];
    }
    if (int rc = sp_check_finite(inv.data(), d, "1 / noise")) return rc;
    if (int rc = sp_check_finite(mw.data(), d, "mean / noise")) return rc;
    ppca_model *m_raw = nullptr;
    if (int rc = ppca_model_create(ctx, d, k, 1.0, A.data(), mw.data(), &m_raw)) return rc;
    const std::unique_ptr<ppca_model, int (*)(ppca_model *)> m(m_raw, ppca_model_free);
    const StatsLayout L(d, m->k);
    if (int rc = ensure(ctx->stats, ctx->stats_cap, sizeof(double) * (size_t)L.len)) return rc;
    double *stats = dptr<double>(ctx->stats);
    ctx->stats_llk_at = -1;  // (the llk in the buffer is the whitened model's: ppca_em_last_llk does not apply)
    std::vector<double> h, hs((size_t)L.len);  // (h: read by the upload, alive until the synchronisation below)
    ppca_sparse view;  // (its two buffers go back to the context's block cache when it leaves scope)
    BufRef abl, cs;
    int rc = sp_upload_abl(ctx, d, inv.data(), mw.data(), nullptr, h, &abl);
    if (!rc) rc = dev_alloc(sizeof(double) * sums.size(), &cs);
    if (!rc) rc = sp_scale(ctx, sp, dptr<const double>(abl), &view, dptr<double>(cs), nullptr);
    if (!rc) rc = sp_accumulate(ctx, &view, m.get(), stats);
    if (!rc && hipMemcpyAsync(sums.data(), cs->p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(hs.data(), stats, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if ((rc = sp_finish(ctx, rc, "FA step"))) return rc;  // the one wait for the results (the upload reads `h`)
    if (int frc = ppca_fa_finalize_host(d, k, noise, transform, mean, hs.data(), sums.data() + (size_t)2 * d, min_noise, noise_out,
                                        transform_out, mean_out))
        return frc;
    if (llk_in) {
        double jac = 0.0;
        for (int j = 0; j < d; ++j) jac += hs[L.totals + j] * std::log(noise[j]);
        *llk_in = hs[L.scalars + SC_LLK] - jac;
    }
    return PPCA_OK;
}
