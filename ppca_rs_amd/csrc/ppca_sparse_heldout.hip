// ppca_sparse_heldout.hip -- hold-out splits and held-out scoring on row-compressed data.  Storage and shared scaffolding:
// ppca_sparse.hpp.
//
// Held-out scoring (ppca_heldout_split_csr_host, ppca_heldout_score_sparse).  The split is host code: entry
// (g, j) draws the word of the dense split (ppca_heldout.hip) and is flagged held iff lo <= u < hi.  The score takes two datasets of
// equal n, d and block_rows, so that block b of `train` and block b of `held` cover the same rows.  Per block: sparse_row_kernel<K>
// writes z and Sigma of train's rows to scratch, then
// sparse_held_row_kernel<K>  runs over held's CSR with held's row lists and the groups of the row pass (W = 4 / 16 / 64 by the HELD
//     row's length).  Lane s takes the row's held entries s, s + W, ..., computes l of each (held_entry<K>: m, v by the k^2
//     multiply-adds of sparse_predict_kernel, in its order) and adds them in that order; one butterfly adds the lanes.  per_row of a
//     row depends on its train entry list (z, Sigma) and its held entry list alone.
// sparse_held_col_kernel<K>  runs over held's inverted index and work items.  An item belongs to a group of 16 lanes; lane s takes
//     the entries s, s + 16, ... of the item (ascending row), recomputes (m, v) from the row's (z, Sigma) with the same held_entry<K>
//     and forms [w | w l | w e^2 | w e^2 / v] (w: train's weight of the row).  Each chunk of 16 entries is added by one butterfly and
//     the chunks in order: a sum is a fixed function of the item's entry list.  A whole column adds into the 4 x d sums (blocks in
//     stream order); a run writes a partial and sparse_colsum_fix_kernel<4> adds a column's runs in run order.  No float atomics.
#include <cmath>
#include <cstring>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

// ---- held-out scoring
// One held entry x of column j (cj = c_j, muj = mean_j) in a row whose posterior given `train` is (z, S): e^2, v and l of the new
// reading.  m and v are sparse_predict_kernel's, multiply-add for multiply-add; l is heldout_score_kernel's expression.
template <int K>
__device__ __forceinline__ void held_entry(const double *cj, const double *z, const double *S, double x, double muj, double s2, double &e2,
                                           double &v, double &l) {
    double c[K];
#pragma unroll
    for (int t = 0; t < K; ++t) c[t] = cj[t];
    double dot = 0.0, q = 0.0;
    // One row of S at a time, the rows in a rolled loop: unrolled, the compiler keeps all K^2 elements of a row's S in registers across
    // the entries of sparse_held_row_kernel (512 VGPRs and spills from K = 15 on).
#pragma unroll 1
    for (int t = 0; t < K; ++t) {
        const double ct = cj[t];
        dot = fma(ct, z[t], dot);
        double sc = 0.0;
#pragma unroll
        for (int u = 0; u < K; ++u) sc = fma(S[t * K + u], c[u], sc);
        q = fma(ct, sc, q);
    }
    const double e = x - (muj + dot);
    e2 = __dmul_rn(e, e);
    v = q + s2;
    l = -0.5 * (LOG_2PI + log(v) + e2 / v);
}

struct SpHeldRowArgs {
    const int64_t *row_ptr;  // held's CSR
    const int32_t *col;
    const double *val;
    const int32_t *rows;  // a bin of held's rows, local to the block
    int64_t nrows, row0;
    int W, d;
    const double *model;
    const double *states, *covs;  // of train's rows, indexed by the row within the block
    double *per_row;              // indexed by global row
};

template <int K>
__global__ __launch_bounds__(256) void sparse_held_row_kernel(SpHeldRowArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1];
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        const double *z = a.states + lr * K, *S = a.covs + lr * (K * K);
        double lsum = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            double e2, v, l;
            held_entry<K>(C + (int64_t)j * K, z, S, a.val[e], mu[j], s2, e2, v, l);
            lsum += l;
        }
        // the group's lanes, one butterfly: the same tree for every row of the bin
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
            if (o < W) lsum += __shfl_xor(lsum, o, 64);
        if (live && sub == 0) a.per_row[r] = lsum;
    }
}

constexpr int SP_HELD_GW = 16;  // lanes of an item's group in sparse_held_col_kernel
constexpr int SP_HELD_NO = 4;   // sums per column: w | w l | w e^2 | w e^2 / v

struct SpHeldColArgs {
    const SpItem *items;  // held's work items, inverted index
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *w;  // train's weights (nullable), indexed by global row
    int64_t row0;
    const double *states, *covs;  // of train's rows, indexed by the row within the block
    const double *model;
    int d;
    double *colsum;  // 4 x d
    double *runpart;
};

template <int K>
__global__ __launch_bounds__(256) void sparse_held_col_kernel(SpHeldColArgs a) {
    constexpr int GW = SP_HELD_GW, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1];
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double *cj = C + (int64_t)it.col * K;
        const double muj = mu[it.col];
        double acc[SP_HELD_NO] = {0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group) one chunk of GW entries, ascending row
            double p[SP_HELD_NO] = {0.0, 0.0, 0.0, 0.0};  // (past the end: exact zeros, which change no sum)
            if (t + sub < it.len) {
                const int64_t li = a.trow[it.start + t + sub];
                const double w = a.w ? a.w[a.row0 + li] : 1.0;
                double e2, v, l;
                held_entry<K>(cj, a.states + li * K, a.covs + li * (K * K), a.tval[it.start + t + sub], muj, s2, e2, v, l);
                p[0] = w;
                p[1] = w * l;
                p[2] = w * e2;
                p[3] = w * (e2 / v);
            }
#pragma unroll
            for (int o = 1; o < GW; o <<= 1)
#pragma unroll
                for (int q = 0; q < SP_HELD_NO; ++q) p[q] += __shfl_xor(p[q], o, 64);
#pragma unroll
            for (int q = 0; q < SP_HELD_NO; ++q) acc[q] += p[q];
        }
        if (live && sub < SP_HELD_NO) {
            const double s = sub == 0 ? acc[0] : sub == 1 ? acc[1] : sub == 2 ? acc[2] : acc[3];
            if (it.dest < 0)
                a.colsum[(int64_t)sub * a.d + it.col] += s;
            else
                a.runpart[it.dest * SP_HELD_NO + sub] = s;
        }
    }
}

}  // namespace ppca_sp

namespace {

template <int K>
hipError_t held_row_t(const SpHeldRowArgs &a, int grid, hipStream_t s) { return sp_launch(sparse_held_row_kernel<K>, grid, s, a); }
template <int K>
hipError_t held_col_t(const SpHeldColArgs &a, int n_cu, hipStream_t s) {
    return sp_launch(sparse_held_col_kernel<K>, sp_grid(a.n_items, 4 * (64 / SP_HELD_GW), n_cu, 8), s, a);
}
hipError_t launch_held_row(int k, const SpHeldRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, held_row_t, a, grid, s); }
hipError_t launch_held_col(int k, const SpHeldColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, held_col_t, a, n_cu, s); }

}  // namespace

extern "C" int ppca_heldout_split_csr_host(int64_t n, const int64_t *row_ptr, const int32_t *col, double lo, double hi, uint64_t seed,
                                           int64_t row_offset, uint8_t *held_flag_out, int64_t *counts_out) {
    if (n < 0 || !row_ptr) return fail(PPCA_ERR_INVALID, "bad shape or null row_ptr");
    if (!(lo >= 0.0 && lo <= hi && hi <= 1.0)) return fail(PPCA_ERR_INVALID, "the range must satisfy 0 <= lo <= hi <= 1");
    if (row_offset < 0) return fail(PPCA_ERR_INVALID, "row_offset must be >= 0");
    if (row_ptr[0] != 0) return fail(PPCA_ERR_INVALID, "row_ptr must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(PPCA_ERR_INVALID, "row_ptr is not monotone at row %lld", (long long)i);
    if (row_ptr[n] > 0 && (!col || !held_flag_out)) return fail(PPCA_ERR_INVALID, "null col or output");
    int64_t held = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = row_key(seed, STREAM_HOLDOUT, (uint64_t)(row_offset + i));
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0) return fail(PPCA_ERR_INVALID, "column %d of row %lld is negative", col[e], (long long)i);
            const double u = u01_floor(row_word(key, (uint64_t)col[e]));
            const bool hold = u >= lo && u < hi;
            held_flag_out[e] = hold ? 1 : 0;
            held += hold ? 1 : 0;
        }
    }
    if (counts_out) {
        counts_out[0] = row_ptr[n] - held;
        counts_out[1] = held;
    }
    return PPCA_OK;
}

extern "C" int ppca_heldout_score_sparse(ppca_ctx *ctx, ppca_sparse *train, ppca_sparse *held, const ppca_model *model, double *totals_host,
                                         double *col_sums_host, double *per_row) {
    if (!held || !totals_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, train, model)) return rc;
    const SpCore &tc = *train->core, &hc = *held->core;
    if (tc.n != hc.n || tc.d != hc.d)
        return fail(PPCA_ERR_INVALID, "the train part (%lld x %d) and the held part (%lld x %d) differ in shape", (long long)tc.n, tc.d,
                    (long long)hc.n, hc.d);
    if (train->ctx->device != held->ctx->device) return fail(PPCA_ERR_INVALID, "the two datasets live on different devices");
    if (tc.block_rows != hc.block_rows)
        return fail(PPCA_ERR_INVALID, "the train part is tiled in blocks of %lld rows and the held part in blocks of %lld: build both with one "
                    "block_rows", (long long)tc.block_rows, (long long)hc.block_rows);
    USE_CTX(ctx);
    const int k = model->k, d = tc.d;
    const int64_t n = tc.n;
    BufRef st, cv, rows, sums, runpart;
    if (int rc = dev_alloc(sizeof(double) * (size_t)tc.max_rows * k, &st)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)tc.max_rows * k * k, &cv)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)n, &rows)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)SP_HELD_NO * d, &sums)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(hc.max_runs, 1) * SP_HELD_NO, &runpart)) return rc;
    double *stp = dptr<double>(st), *cvp = dptr<double>(cv), *rowv = dptr<double>(rows), *colsum = dptr<double>(sums), *runs = dptr<double>(runpart);
    HIP_TRY(hipMemsetAsync(rowv, 0, sizeof(double) * (size_t)n, ctx->stream));
    HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(double) * (size_t)SP_HELD_NO * d, ctx->stream));
    for (size_t bi = 0; bi < hc.blocks.size(); ++bi) {
        const SpBlock &tb = tc.blocks[bi], &hb = hc.blocks[bi];  // (the same rows: equal n and block_rows)
        if (hb.nnz == 0) continue;                               // nothing held in these rows: their scores stay 0
        if (int rc = sp_rows_of_block(ctx, train, tb, model, nullptr, stp, cvp, nullptr, nullptr)) return rc;
        SpHeldRowArgs ra{};
        ra.d = d;
        ra.model = model->p();
        ra.states = stp;
        ra.covs = cvp;
        ra.per_row = rowv;
        const auto row = [&](const SpHeldRowArgs &a, int grid) { return launch_held_row(k, a, grid, ctx->stream); };
        if (int rc = sp_for_bins(ctx, held, hb, ra, row)) return rc;
        SpHeldColArgs ca{};
        ca.w = train->w;
        ca.row0 = hb.row0;
        ca.states = stp;
        ca.covs = cvp;
        ca.model = model->p();
        ca.colsum = colsum;
        const auto item = [&](const SpHeldColArgs &a) { return launch_held_col(k, a, ctx->n_cu, ctx->stream); };
        const auto fix = [&] { return sp_colsum_fix<SP_HELD_NO>(ctx, hb, runs, d, colsum); };
        if (int rc = sp_col_pass(held, hb, runs, ca, item, fix)) return rc;
    }
    std::vector<double> cs((size_t)SP_HELD_NO * d);
    HIP_TRY(hipMemcpyAsync(cs.data(), colsum, sizeof(double) * cs.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (per_row) HIP_TRY(hipMemcpyAsync(per_row, rowv, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < SP_HELD_NO; ++q) {  // the column sums added in index order, as ppca_heldout_score's totals
        double s = 0.0;
        for (int j = 0; j < d; ++j) s += cs[(size_t)q * d + j];
        totals_host[q] = s;
    }
    totals_host[4] = (double)hc.nnz;
    totals_host[5] = (double)hc.nonempty_rows;
    if (col_sums_host) std::memcpy(col_sums_host, cs.data(), sizeof(double) * cs.size());
    return PPCA_OK;
}
