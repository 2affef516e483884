// ppca_sparse_hetero.hip -- PPCA with a known precision per entry on row-compressed data (HPPCAModel on a SparseDataset; DESIGN.md
// section 4.30): x_ij = mean_j + c_j . z_i + eps_ij, eps_ij ~ N(0, sigma^2 / p_ij), on the entries that are stored.  Every stored
// entry has a precision that is finite and > 0 (an entry that should not count is not stored: there is no masking precision here).
// Storage, the values view and the shared scaffolding: ppca_sparse.hpp.
//
// The precisions are a values view of the dataset (ppca_h_sparse_precisions): the pattern, row lists, inverted index and work items
// are the dataset's, the view's two buffers hold p in CSR order (uploaded) and in index order (sparse_h_fill_kernel).  No pattern is
// compared on the device: a pass takes the view of the dataset it is given (the same core), else PPCA_ERR_INVALID.
//
// sparse_h_fill_kernel   the index-order precisions.  The work items and 16-lane groups of sparse_scale_col_kernel; for the item's
//     entry (column j, row i) the lane bisects row i's strictly increasing column list for j and copies that position's precision.
// sparse_h_row_kernel<K> sparse_row_kernel<K> with a precision per entry: the same groups of W = 4 / 16 / 64 lanes by bin, lane s
//     takes the entries s, s + W, ..., one butterfly, Posterior<K>.  The sums are G = sum p c c^T, b = sum p x~ c, sum p x~^2 and
//     sum ln p, the last as a product of mantissas and a sum of exponents (frexp, renormalised at every entry) with one logarithm
//     per lane.  Outputs, all nullable: ell, z, Sigma, the record [w z | w | w (Sigma + z z^T) packed], the row's three scalar terms.
// sparse_h_scal_kernel   the scalar terms of a block, 1024 rows per workgroup in a fixed tree (sparse_scal_kernel's).
// sparse_h_col_kernel<K> sparse_col_kernel<K> with a precision per entry: lane o of an item's group owns output o of the column's
//     2 k + k' + 4 sums and adds the item's entries in ascending row.  With r the row's record and (x~, p) the entry:
//         o in [0, NR)            p r[o]                 V (k) | T | S (k')
//         o in [NR, NR + k + 1)   p x~ r[o - NR]         cross (k) | A
//         o = NR + k + 1          p x~^2 r[k]            sq                     o = NR + k + 2     r[k]      cnt
//     A whole column adds into the statistics (blocks in stream order), a run writes its partial and sparse_h_fix_kernel adds a
//     column's runs in run order.  No float atomics.
//
// ell, z and Sigma of a row depend on its entry list alone; the statistics are bit-identical under any grid limit for a given
// (block_rows, segment).  The statistics buffer is ppca_h_estep's (cross | S | V | A | T | sq | cnt) and lives in scratch of the
// pass's own: the context's statistics buffer and ppca_em_last_llk are not touched.
#include <cmath>
#include <cstring>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

constexpr int SP_H_FILL_GW = 16;  // lanes of an item's group in sparse_h_fill_kernel
constexpr int SP_H_NSCAL = 3;     // per-row scalar terms: w | w ell | non-empty

struct SpHFillArgs {
    const SpItem *items;
    int64_t n_items;
    const int32_t *trow;
    const double *tval;  // (the dataset's: not read)
    int d;
    double *runpart;     // (not used)
    const int64_t *row_ptr;
    const int32_t *col;
    const double *prec;  // CSR order
    int64_t row0;
    double *out_tprec;   // index order
};

// Index entry `at` of an item is (column it.col, row row0 + trow[at]).  Its precision sits in CSR order at the position of it.col in
// the row's column list, which is strictly increasing: a bisection over [row_ptr[r], row_ptr[r + 1]), at most 31 halvings (a row
// holds fewer than 2^31 entries).  Every index entry belongs to exactly one item: the kernel writes all of out_tprec.
__global__ __launch_bounds__(256) void sparse_h_fill_kernel(SpHFillArgs a) {
    constexpr int GW = SP_H_FILL_GW, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        for (int t = sub; t < it.len; t += GW) {
            const int64_t at = it.start + t;
            const int64_t r = a.row0 + a.trow[at];
            int64_t lo = a.row_ptr[r], hi = a.row_ptr[r + 1];
            double p = __builtin_nan("");  // (a column the row does not hold: cannot happen on a container that was validated)
            if (hi > lo) {
                for (int step = 0; step < 31 && hi - lo > 1; ++step) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (a.col[mid] <= it.col)
                        lo = mid;
                    else
                        hi = mid;
                }
                if (a.col[lo] == it.col) p = a.prec[lo];
            }
            a.out_tprec[at] = p;
        }
    }
}

struct SpHRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const double *prec;   // CSR order
    const double *w;      // nullable, indexed by global row
    const int32_t *rows;  // the bin's rows, local to the block
    int64_t nrows, row0;
    int W, d;
    const double *model;
    double *llks, *states, *covs, *rec, *rscal;  // nullable, indexed by the row within the block
};

template <int K>
__global__ __launch_bounds__(256) void sparse_h_row_kernel(SpHRowArgs a) {
    constexpr int KP = K * (K + 1) / 2, NR = K + 1 + KP;
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1], lnsig = a.model[2];
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        double G[KP], b[K], xx = 0.0, slm = 1.0;
        int sle = 0;
#pragma unroll
        for (int e = 0; e < KP; ++e) G[e] = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) b[t] = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            const double p = a.prec[e];
            const double xt = a.val[e] - mu[j];
            const double *cj = C + (int64_t)j * K;
            double c[K], pc[K];
#pragma unroll
            for (int t = 0; t < K; ++t) {
                c[t] = cj[t];
                pc[t] = __dmul_rn(p, c[t]);
            }
            xx = fma(__dmul_rn(p, xt), xt, xx);
            {  // the product of the precisions as mantissa x 2^exponent: the mantissa stays in [1/2, 1)
                int ep = 0, em = 0;
                slm = __builtin_frexp(slm * __builtin_frexp(p, &ep), &em);
                sle += ep + em;
            }
#pragma unroll
            for (int t = 0; t < K; ++t) {
                b[t] = fma(xt, pc[t], b[t]);
#pragma unroll
                for (int u = 0; u <= t; ++u) G[tri(t, u)] = fma(pc[t], c[u], G[tri(t, u)]);
            }
        }
        double sl = log(slm) + (double)sle * LN_2;  // the lane's sum of ln p (0 on a lane without an entry)
        // the group's lanes, one butterfly: the same tree for every row of the bin, the same sums on every lane
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            if (o < W) {
#pragma unroll
                for (int e = 0; e < KP; ++e) G[e] += __shfl_xor(G[e], o, 64);
#pragma unroll
                for (int t = 0; t < K; ++t) b[t] += __shfl_xor(b[t], o, 64);
                xx += __shfl_xor(xx, o, 64);
                sl += __shfl_xor(sl, o, 64);
            }
        }
        const int m = (int)(e1 - e0);
        Posterior<K> post;
        double pm;
        int pe;
        post.factor([&](int e) { return G[e]; }, s2, pm, pe);
        double z[K], quad, zz;
        post.solve([&](int t) { return b[t]; }, z, quad, zz);
        const double ell = m > 0 ? sample_llk(xx, quad, Posterior<K>::logdet(pm, pe), s2, lnsig, m, K) + 0.5 * sl : 0.0;
        const double w = (live && a.w) ? a.w[r] : 1.0;
        double *rec = (live && a.rec) ? a.rec + lr * NR : nullptr;
        double *cov = (live && a.covs) ? a.covs + lr * (K * K) : nullptr;
        if (a.covs || a.rec) {  // (uniform; llk alone needs no M^-1) the columns of M^-1, shared among the group's lanes
            for (int c = sub; c < K; c += W) {
                double zc = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) zc = t == c ? z[t] : zc;
                post.minv_column(c, [&](int t, int cc, double v) {
                    const double sg = s2 * v;
                    if (cov) {
                        cov[t * K + cc] = sg;
                        cov[cc * K + t] = sg;
                    }
                    if (rec) rec[K + 1 + tri(t, cc)] = w * fma(z[t], zc, sg);
                });
            }
        }
        if (live && sub == 0) {
            if (a.llks) a.llks[lr] = ell;
            if (a.states) {
#pragma unroll
                for (int t = 0; t < K; ++t) a.states[lr * K + t] = z[t];
            }
            if (rec) {
#pragma unroll
                for (int t = 0; t < K; ++t) rec[t] = w * z[t];
                rec[K] = w;
            }
            if (a.rscal) {
                double *sc = a.rscal + lr * SP_H_NSCAL;
                sc[0] = w;
                sc[1] = w * ell;
                sc[2] = m > 0 ? 1.0 : 0.0;
            }
        }
    }
}

// part[blockIdx][4] = the sums of the scalar terms of rows [1024 blockIdx, ...) | 0: thread t adds rows t, t + 256, .. in order, then
// a fixed tree over the threads
__global__ __launch_bounds__(256) void sparse_h_scal_kernel(const double *rscal, int64_t rows, double *part) {
    __shared__ double red[256][SP_H_NSCAL];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SP_SCAL_ROWS;
    double s[SP_H_NSCAL] = {0, 0, 0};
    for (int i = 0; i < SP_SCAL_ROWS / 256; ++i) {
        const int64_t r = r0 + tid + 256 * i;
        if (r < rows) {
#pragma unroll
            for (int q = 0; q < SP_H_NSCAL; ++q) s[q] += rscal[r * SP_H_NSCAL + q];
        }
    }
#pragma unroll
    for (int q = 0; q < SP_H_NSCAL; ++q) red[tid][q] = s[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < SP_H_NSCAL; ++q) red[tid][q] += red[tid + o][q];
        }
        __syncthreads();
    }
    if (tid < 4) part[(int64_t)blockIdx.x * 4 + tid] = tid < SP_H_NSCAL ? red[0][tid] : 0.0;
}

template <int K>
struct SpHColCfg {
    static constexpr int KP = K * (K + 1) / 2, NR = K + 1 + KP, NO = NR + K + 3;
    static constexpr int GW = NO <= 8 ? 8 : NO <= 16 ? 16 : NO <= 32 ? 32 : 64;
    static constexpr int EPL = (NO + GW - 1) / GW;
};
__host__ __device__ inline int sp_h_no(int k) { return k * (k + 1) / 2 + 2 * k + 4; }
// where output o of column j lives in the statistics of ppca_h_estep: cross (d x k) | S (d x k') | V (d x k) | A | T | sq | cnt
__device__ __forceinline__ int64_t sp_h_stat_index(int o, int j, int d, int k) {
    const int kp = k * (k + 1) / 2, nr = k + 1 + kp;
    const int64_t oS = (int64_t)d * k, oV = oS + (int64_t)d * kp, oA = oV + (int64_t)d * k, oT = oA + d, oQ = oT + d, oC = oQ + d;
    if (o < k) return oV + (int64_t)j * k + o;
    if (o == k) return oT + j;
    if (o < nr) return oS + (int64_t)j * kp + (o - k - 1);
    if (o - nr < k) return (int64_t)j * k + (o - nr);
    if (o - nr == k) return oA + j;
    return o - nr == k + 1 ? oQ + j : oC + j;
}

struct SpHColArgs {
    const SpItem *items;
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *tprec;  // index order
    const double *rec;    // the block's records
    const double *model;
    int d;
    double *stats, *runpart;
};

template <int K>
__global__ __launch_bounds__(256) void sparse_h_col_kernel(SpHColArgs a) {
    using Cf = SpHColCfg<K>;
    constexpr int GW = Cf::GW, NR = Cf::NR, NO = Cf::NO, EPL = Cf::EPL, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1), gbase = lane & ~(GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double *mu = a.model + MODEL_HDR + (int64_t)a.d * K;
    // what output o reads of the record, and which of p | p x~ | p x~^2 | 1 multiplies it
    int src[EPL], sel[EPL];
#pragma unroll
    for (int q = 0; q < EPL; ++q) {
        const int o = sub + q * GW;
        src[q] = o < NR ? o : o < NR + K + 1 ? o - NR : K;
        sel[q] = o < NR ? 0 : o < NR + K + 1 ? 1 : o == NR + K + 1 ? 2 : 3;
    }
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double muj = mu[it.col];
        double acc[EPL];
#pragma unroll
        for (int q = 0; q < EPL; ++q) acc[q] = 0.0;
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group)
            const bool mine = t + sub < it.len;
            const int li = mine ? a.trow[it.start + t + sub] : 0;
            const double xv = mine ? a.tval[it.start + t + sub] - muj : 0.0;
            const double pv = mine ? a.tprec[it.start + t + sub] : 0.0;
            const int nb = it.len - t < GW ? it.len - t : GW;
            for (int q = 0; q < nb; q += 4) {  // the entries in ascending row, four record gathers in flight
                double f[4][4], v[4][EPL];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int from = gbase + ((q + u) & (GW - 1));
                    const int i = __shfl(li, from, 64);
                    const double x = __shfl(xv, from, 64), p = __shfl(pv, from, 64);
                    f[u][0] = p;
                    f[u][1] = __dmul_rn(p, x);
                    f[u][2] = __dmul_rn(f[u][1], x);
                    f[u][3] = 1.0;
                    const bool ok = q + u < nb;  // (past the end: exact zeros, which change no sum)
                    const double *rr = a.rec + (int64_t)i * NR;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) v[u][e] = (ok && sub + e * GW < NO) ? rr[src[e]] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        const double fm = sel[e] == 0 ? f[u][0] : sel[e] == 1 ? f[u][1] : sel[e] == 2 ? f[u][2] : f[u][3];
                        acc[e] = fma(fm, v[u][e], acc[e]);
                    }
            }
        }
        if (live) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int o = sub + e * GW;
                if (o >= NO) continue;
                if (it.dest < 0) {
                    double *dst = a.stats + sp_h_stat_index(o, it.col, a.d, K);
                    *dst += acc[e];
                } else {
                    a.runpart[it.dest * NO + o] = acc[e];
                }
            }
        }
    }
}

// statistics of a long column += its runs' partials, added in run order
__global__ __launch_bounds__(256) void sparse_h_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, int k, double *stats) {
    const int no = sp_h_no(k);
    for (int64_t c = blockIdx.x; c < n_long; c += gridDim.x) {
        const SpLong lc = longs[c];
        for (int o = threadIdx.x; o < no; o += blockDim.x) {
            double s = 0.0;
            for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * no + o];
            stats[sp_h_stat_index(o, lc.col, d, k)] += s;
        }
    }
}

}  // namespace ppca_sp

namespace {

template <int K>
hipError_t h_row_t(const SpHRowArgs &a, int grid, hipStream_t s) { return sp_launch(sparse_h_row_kernel<K>, grid, s, a); }
template <int K>
hipError_t h_col_t(const SpHColArgs &a, int n_cu, hipStream_t s) {
    return sp_launch(sparse_h_col_kernel<K>, sp_grid(a.n_items, 4 * (64 / SpHColCfg<K>::GW), n_cu, 8), s, a);
}
hipError_t launch_h_row(int k, const SpHRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, h_row_t, a, grid, s); }
hipError_t launch_h_col(int k, const SpHColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, h_col_t, a, n_cu, s); }

int64_t sp_h_stats_len(int d, int k) { return (int64_t)d * sp_h_no(k); }

// the model, the dataset and its precisions of a pass: everything that is checked before a device is touched
int sp_h_check(const ppca_ctx *ctx, const ppca_sparse *sp, const ppca_sparse *prec, const ppca_model *model) {
    if (!prec) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, sp, model)) return rc;
    if (model->k_user() < 1)
        return fail(PPCA_ERR_UNSUPPORTED, "state size 0 is not supported by the known-precision model on sparse data: the kernels cover 1 <= k <= %d",
                    SP_MAX_K);
    if (prec->core != sp->core || !prec->vbuf || !prec->tvbuf)
        return fail(PPCA_ERR_INVALID, "the precisions are not a view of this dataset's pattern (ppca_h_sparse_precisions)");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    return PPCA_OK;
}

// the row pass (sparse_h_row_kernel<k>) over one block: outputs, all nullable, indexed by the row within the block
int sp_h_rows_of_block(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_sparse *prec, const SpBlock &b, const ppca_model *model, double *llks,
                       double *states, double *covs, double *rec, double *rscal) {
    SpHRowArgs a{};
    a.prec = prec->val();
    a.w = sp->w;
    a.d = sp->core->d;
    a.model = model->p();
    a.llks = llks;
    a.states = states;
    a.covs = covs;
    a.rec = rec;
    a.rscal = rscal;
    const auto row = [&](const SpHRowArgs &ba, int grid) { return launch_h_row(model->k, ba, grid, ctx->stream); };
    return sp_for_bins(ctx, sp, b, a, row);
}

// What an E-step keeps alive until the caller's synchronisation: scratch of the pass's own.
struct SpHSweep {
    BufRef llks, states, covs, rec, rscal, spart, runpart, stats, scal;
};

// Enqueues the E-step of sp under (model, prec) block by block.  llks (nullable, n, device): filled here.  states_out / covs_out
// (nullable): destinations of hipMemcpyDefault, n x k and n x k x k, copied block by block from one block's scratch (with a wait per
// block: the next block overwrites it).  want_stats: the statistics of ppca_h_estep into sw.stats.  The scalars sum w | sum w ell |
// rows with an entry | 0 go to sw.scal (4 doubles).  Without states_out / covs_out there is no wait.
int sp_h_sweep(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_sparse *prec, const ppca_model *model, double *llks, double *states_out,
               double *covs_out, bool want_stats, SpHSweep &sw) {
    const SpCore &c = *sp->core;
    const int k = model->k, nr = k + 1 + k * (k + 1) / 2;
    const size_t rows = (size_t)std::max<int64_t>(c.max_rows, 1);
    if (int rc = dev_alloc(sizeof(double) * rows * SP_H_NSCAL, &sw.rscal)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 4 * ((rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS), &sw.spart)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 4, &sw.scal)) return rc;
    HIP_TRY(hipMemsetAsync(sw.scal->p, 0, sizeof(double) * 4, ctx->stream));
    if (states_out)
        if (int rc = dev_alloc(sizeof(double) * rows * k, &sw.states)) return rc;
    if (covs_out)
        if (int rc = dev_alloc(sizeof(double) * rows * k * k, &sw.covs)) return rc;
    double *stats = nullptr, *rec = nullptr, *runpart = nullptr;
    if (want_stats) {
        const size_t slen = (size_t)sp_h_stats_len(c.d, k);
        if (int rc = dev_alloc(sizeof(double) * slen, &sw.stats)) return rc;
        if (int rc = dev_alloc(sizeof(double) * rows * nr, &sw.rec)) return rc;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * sp_h_no(k), &sw.runpart)) return rc;
        stats = dptr<double>(sw.stats);
        rec = dptr<double>(sw.rec);
        runpart = dptr<double>(sw.runpart);
        HIP_TRY(hipMemsetAsync(stats, 0, sizeof(double) * slen, ctx->stream));
    }
    double *st = sw.states ? dptr<double>(sw.states) : nullptr, *cv = sw.covs ? dptr<double>(sw.covs) : nullptr;
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_h_rows_of_block(ctx, sp, prec, b, model, llks ? llks + b.row0 : nullptr, st, cv, rec, dptr<double>(sw.rscal))) return rc;
        const int parts = (int)((b.rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS);
        HIP_TRY(sp_launch(sparse_h_scal_kernel, parts, ctx->stream, dptr<const double>(sw.rscal), b.rows, dptr<double>(sw.spart)));
        HIP_TRY(launch_reduce_partials(dptr<double>(sw.spart), parts, 4, dptr<double>(sw.scal), ctx->stream, 1));
        if (want_stats) {
            SpHColArgs ca{};
            ca.tprec = prec->tval();
            ca.rec = rec;
            ca.model = model->p();
            ca.stats = stats;
            const auto item = [&](const SpHColArgs &a) { return launch_h_col(k, a, ctx->n_cu, ctx->stream); };
            const auto fix = [&] {  // one workgroup per long column
                return sp_launch(sparse_h_fix_kernel, sp_grid(b.n_long, 1, ctx->n_cu, 8), ctx->stream, b.longs(), b.n_long, (const double *)runpart,
                                 c.d, k, stats);
            };
            if (int rc = sp_col_pass(sp, b, runpart, ca, item, fix)) return rc;
        }
        if (st) HIP_TRY(hipMemcpyAsync(states_out + b.row0 * k, st, sizeof(double) * (size_t)b.rows * k, hipMemcpyDefault, ctx->stream));
        if (cv) HIP_TRY(hipMemcpyAsync(covs_out + b.row0 * k * k, cv, sizeof(double) * (size_t)b.rows * k * k, hipMemcpyDefault, ctx->stream));
        if (st || cv) HIP_TRY(hipStreamSynchronize(ctx->stream));  // the next block overwrites the scratch
    }
    return PPCA_OK;
}

}  // namespace

extern "C" int ppca_h_sparse_precisions(const double *prec_host, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse **view_out) {
    if (!ctx || !sp || !view_out) return fail(PPCA_ERR_INVALID, "null argument");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    const SpCore &c = *sp->core;
    if (c.nnz > 0 && !prec_host) return fail(PPCA_ERR_INVALID, "null argument");
    for (int64_t e = 0; e < c.nnz; ++e)
        if (!(prec_host[e] > 0.0) || !std::isfinite(prec_host[e]))
            return fail(PPCA_ERR_INVALID, "precision %lld is not a positive finite number (an entry that should not count is not stored)",
                        (long long)e);
    USE_CTX(ctx);
    auto view = std::make_unique<ppca_sparse>();
    view->ctx = sp->ctx;
    view->core = sp->core;
    view->wbuf = sp->wbuf;
    view->w = sp->w;
    int rc = sp_upload(ctx, prec_host, sizeof(double) * (size_t)c.nnz, &view->vbuf);
    if (!rc) rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.nnz, 1), &view->tvbuf);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        SpHFillArgs a{};
        a.row_ptr = c.row_ptr();
        a.col = c.col();
        a.prec = dptr<const double>(view->vbuf);
        a.row0 = b.row0;
        a.out_tprec = dptr<double>(view->tvbuf);
        const auto item = [&](const SpHFillArgs &fa) {
            return sp_launch(sparse_h_fill_kernel, sp_grid(fa.n_items, 4 * (64 / SP_H_FILL_GW), ctx->n_cu, 8), ctx->stream, fa);
        };
        rc = sp_col_pass(sp, b, nullptr, a, item, [] { return hipSuccess; });
    }
    if ((rc = sp_finish(ctx, rc, "precision view"))) return rc;  // (the upload reads the caller's buffer)
    *view_out = view.release();
    return PPCA_OK;
}

extern "C" int ppca_h_sparse_estep(const ppca_model *model, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse *prec, double *llks, double *states,
                                   double *covs, double *stats_host, double *scalars_host) {
    if (!llks && !states && !covs && !stats_host && !scalars_host) return fail(PPCA_ERR_INVALID, "no output requested");
    if (int rc = sp_h_check(ctx, sp, prec, model)) return rc;
    USE_CTX(ctx);
    const SpCore &c = *sp->core;
    const int k = model->k;
    SpHSweep sw;
    double h[4] = {0, 0, 0, 0};
    if (llks)
        if (int rc = dev_alloc(sizeof(double) * (size_t)c.n, &sw.llks)) return rc;
    int rc = sp_h_sweep(ctx, sp, prec, model, llks ? dptr<double>(sw.llks) : nullptr, states, covs, stats_host != nullptr, sw);
    if (!rc && llks && hipMemcpyAsync(llks, sw.llks->p, sizeof(double) * (size_t)c.n, hipMemcpyDefault, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && stats_host &&
        hipMemcpyAsync(stats_host, sw.stats->p, sizeof(double) * (size_t)sp_h_stats_len(c.d, k), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(h, sw.scal->p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(PPCA_ERR_HIP, "download failed");
    if ((rc = sp_finish(ctx, rc, "known-precision E-step"))) return rc;
    if (scalars_host) std::memcpy(scalars_host, h, sizeof(h));
    return PPCA_OK;
}

extern "C" int ppca_h_sparse_em_step(int32_t d, int32_t k, double sigma, const double *transform, const double *mean, ppca_ctx *ctx,
                                     ppca_sparse *sp, ppca_sparse *prec, double *sigma_out, double *transform_out, double *mean_out,
                                     double *llk_in) {
    if (!ctx || !sp || !prec || !transform || !mean || !sigma_out || !transform_out || !mean_out) return fail(PPCA_ERR_INVALID, "null argument");
    if (d < 1 || k < 0) return fail(PPCA_ERR_INVALID, "invalid shape d=%d k=%d", d, k);
    if (sp->core->d != d) return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", sp->core->d, d);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(PPCA_ERR_INVALID, "sigma is not a positive finite number");
    if (k < 1 || k > SP_MAX_K)
        return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported by the known-precision model on sparse data: the kernels cover 1 <= k <= %d",
                    k, SP_MAX_K);
    if (sp->core->n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    if (prec->core != sp->core || !prec->vbuf || !prec->tvbuf)
        return fail(PPCA_ERR_INVALID, "the precisions are not a view of this dataset's pattern (ppca_h_sparse_precisions)");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    USE_CTX(ctx);
    ppca_model *m_raw = nullptr;
    if (int rc = ppca_model_create(ctx, d, k, sigma, transform, mean, &m_raw)) return rc;
    const std::unique_ptr<ppca_model, int (*)(ppca_model *)> m(m_raw, ppca_model_free);
    if (int rc = sp_h_check(ctx, sp, prec, m.get())) return rc;
    std::vector<double> hs((size_t)sp_h_stats_len(d, k));
    double h[4] = {0, 0, 0, 0};
    SpHSweep sw;
    int rc = sp_h_sweep(ctx, sp, prec, m.get(), nullptr, nullptr, nullptr, true, sw);
    if (!rc && hipMemcpyAsync(hs.data(), sw.stats->p, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(h, sw.scal->p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(PPCA_ERR_HIP, "download failed");
    if ((rc = sp_finish(ctx, rc, "known-precision step"))) return rc;  // the one wait for the results
    // (ppca_h_finalize_host's M-step, without that entry's limit on d, which is the dense sweep's)
    if (int frc = h_finalize(d, k, sigma, transform, mean, hs.data(), sigma_out, transform_out, mean_out)) return frc;
    if (llk_in) *llk_in = h[1];
    return PPCA_OK;
}

extern "C" int ppca_h_sparse_predict(const ppca_model *model, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse *prec, const int64_t *query_row_ptr,
                                     const int32_t *query_col, double *mean_host, double *var_host) {
    if (int rc = sp_h_check(ctx, sp, prec, model)) return rc;
    const auto rows = [&](const SpBlock &b, double *states, double *covs) {
        return sp_h_rows_of_block(ctx, sp, prec, b, model, nullptr, states, covs, nullptr, nullptr);
    };
    return sp_predict(ctx, sp, model, query_row_ptr, query_col, mean_host, var_host, rows);
}
