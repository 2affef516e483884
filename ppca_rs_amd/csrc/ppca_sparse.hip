// ppca_sparse.hip -- masked PPCA on row-compressed data (SparseDataset): the container, the host-side inverted
// index, the two passes that produce the packed statistics of include/ppca_hip.h from it, and the entry points that share the row
// pass (llk, infer, predict).  The model, the statistics buffer and the M-step are those of the dense path.  The storage, and what
// the other files of the path share with this one, is in ppca_sparse.hpp; sparse_row_kernel<K> is instantiated here alone, and the
// other files reach it through sp_rows_of_block.
//
// sparse_row_kernel<K>  the E-step over one bin of one block.  A row belongs to a group of W lanes of a wave, W = 4 / 16 / 64 by bin,
//     so short rows share a wave and a long row has one to itself.  Lane s of the group takes the row's entries s, s + W, ... in
//     order, gathers the rows of C by column index and accumulates its own [G | b | |x~|^2]; one butterfly of log2 W steps adds the
//     lanes (the same tree for every row of the bin, the same sum on every lane).  Every lane then factors M = sigma^2 I + G and solves
//     (Posterior<K>, redundantly: the columns of M^-1 are shared among the group's lanes).  W is a function of the row's length, the
//     lane an entry goes to a function of its position in the row: ell, z and Sigma of a row depend on its entry list alone, not on
//     the grid, block_rows or the row's position.  Outputs, all nullable: ell, z, Sigma, the record [w z | w | w (Sigma + z z^T)
//     packed] and the row's five scalar terms.
// sparse_scal_kernel    the scalar terms of a block, 1024 rows per workgroup in a fixed tree; launch_reduce_partials adds the
//     workgroups in order: the eight scalars do not depend on the grid either.
// sparse_col_kernel<K>  the statistics over the inverted index (store the records, then sum per destination: no float atomics).  An
//     item belongs to a group of GW lanes (8 .. 64 by K: short columns are packed several to a wave); lane o of the group owns output o
//     of [U_j | totals_j | S_j | cross_j | sumx_j] (up to three per lane) and adds the item's entries in ascending row, gathering each
//     entry's record from scratch with one coalesced read per group.  A whole column adds its sum to the statistics (the blocks run one
//     after the other on the stream: block order); a run writes its partial, and sparse_fix_kernel adds a column's runs in run order.
// sparse_predict_kernel mean_j + c_j . z_i and c_j^T Sigma_i c_j + sigma^2 per query entry from the states / covariances of the block.
#include <chrono>
#include <climits>
#include <cmath>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

// ------------------------------------------------------------------ kernels
struct SpRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const double *w;      // nullable, indexed by global row
    const int32_t *rows;  // the bin's rows, local to the block
    int64_t nrows, row0;
    int W, d;
    const double *model;
    double *llks, *states, *covs, *rec, *rscal;  // nullable, indexed by the row within the block
};

// (sp_mix_row_ell in ppca_sparse_mix.hip is a second copy of this kernel's sums, tree, factorisation and ell, and promises this kernel's
// bits: change both; tests/test_gpu_sparse_mix.py holds every K to it)
template <int K>
__global__ __launch_bounds__(256) void sparse_row_kernel(SpRowArgs a) {
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
        double G[KP], b[K], xx = 0.0;
#pragma unroll
        for (int e = 0; e < KP; ++e) G[e] = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) b[t] = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            const double xt = a.val[e] - mu[j];
            const double *cj = C + (int64_t)j * K;
            double c[K];
#pragma unroll
            for (int t = 0; t < K; ++t) c[t] = cj[t];
            xx = fma(xt, xt, xx);
#pragma unroll
            for (int t = 0; t < K; ++t) {
                b[t] = fma(xt, c[t], b[t]);
#pragma unroll
                for (int u = 0; u <= t; ++u) G[tri(t, u)] = fma(c[t], c[u], G[tri(t, u)]);
            }
        }
        // the group's lanes, one butterfly: the same tree for every row of the bin, the same sums on every lane
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            if (o < W) {
#pragma unroll
                for (int e = 0; e < KP; ++e) G[e] += __shfl_xor(G[e], o, 64);
#pragma unroll
                for (int t = 0; t < K; ++t) b[t] += __shfl_xor(b[t], o, 64);
                xx += __shfl_xor(xx, o, 64);
            }
        }
        const int m = (int)(e1 - e0);
        Posterior<K> post;
        double pm;
        int pe;
        post.factor([&](int e) { return G[e]; }, s2, pm, pe);
        double z[K], quad, zz;
        post.solve([&](int t) { return b[t]; }, z, quad, zz);
        const double ell = sample_llk(xx, quad, Posterior<K>::logdet(pm, pe), s2, lnsig, m, K);
        const double w = (live && a.w) ? a.w[r] : 1.0;
        double *rec = (live && a.rec) ? a.rec + lr * NR : nullptr;
        double *cov = (live && a.covs) ? a.covs + lr * (K * K) : nullptr;
        double trace = 0.0;
        if (a.covs || a.rec) {  // (uniform; llk alone needs no M^-1) the columns of M^-1, shared among the group's lanes
            for (int c = sub; c < K; c += W) {
                double zc = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) zc = t == c ? z[t] : zc;
                trace += post.minv_column(c, [&](int t, int cc, double v) {
                    const double sg = s2 * v;
                    if (cov) {
                        cov[t * K + cc] = sg;
                        cov[cc * K + t] = sg;
                    }
                    if (rec) rec[K + 1 + tri(t, cc)] = w * fma(z[t], zc, sg);
                });
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
                if (o < W) trace += __shfl_xor(trace, o, 64);
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
                double *sc = a.rscal + lr * SP_NSCAL;
                // sigma^2 tr(I - sigma^2 M^-1) = tr(Sigma C_o^T C_o); read by the EM pass only (without a record there is no trace)
                sc[0] = m > 0 ? w * (s2 * ((double)K - s2 * trace)) : 0.0;
                sc[1] = m > 0 ? w * (xx - quad - s2 * zz) : 0.0;            // |x~ - C_o z|^2
                sc[2] = w * ell;
                sc[3] = w;
                sc[4] = m > 0 ? 1.0 : 0.0;
            }
        }
    }
}

// part[blockIdx][8] = the sums of the scalar terms of rows [1024 blockIdx, ...): thread t adds rows t, t + 256, .. in order, then a
// fixed tree over the threads
__global__ __launch_bounds__(256) void sparse_scal_kernel(const double *rscal, int64_t rows, double *part) {
    __shared__ double red[256][SP_NSCAL];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SP_SCAL_ROWS;
    double s[SP_NSCAL] = {0, 0, 0, 0, 0};
    for (int i = 0; i < SP_SCAL_ROWS / 256; ++i) {
        const int64_t r = r0 + tid + 256 * i;
        if (r < rows) {
#pragma unroll
            for (int q = 0; q < SP_NSCAL; ++q) s[q] += rscal[r * SP_NSCAL + q];
        }
    }
#pragma unroll
    for (int q = 0; q < SP_NSCAL; ++q) red[tid][q] = s[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int q = 0; q < SP_NSCAL; ++q) red[tid][q] += red[tid + o][q];
        }
        __syncthreads();
    }
    if (tid < 8) part[(int64_t)blockIdx.x * 8 + tid] = tid < SP_NSCAL ? red[0][tid] : 0.0;
}

template <int K>
struct SpColCfg {
    static constexpr int KP = K * (K + 1) / 2, NR = K + 1 + KP, NO = NR + K + 1;
    static constexpr int GW = NO <= 8 ? 8 : NO <= 16 ? 16 : NO <= 32 ? 32 : 64;
    static constexpr int EPL = (NO + GW - 1) / GW;
};
__host__ __device__ inline int sp_no(int k) { return k * (k + 1) / 2 + 2 * k + 2; }
// where output o of column j lives in the packed statistics
__device__ __forceinline__ int64_t sp_stat_index(int o, int j, int d, int k) {
    const int kp = k * (k + 1) / 2, nr = k + 1 + kp;
    const int64_t oS = (int64_t)d * k, oU = oS + (int64_t)d * kp, oX = oU + (int64_t)d * k, oT = oX + d;
    if (o < k) return oU + (int64_t)j * k + o;
    if (o == k) return oT + j;
    if (o < nr) return oS + (int64_t)j * kp + (o - k - 1);
    if (o - nr < k) return (int64_t)j * k + (o - nr);
    return oX + j;
}

struct SpColArgs {
    const SpItem *items;
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *rec;  // the block's records
    const double *model;
    int d;
    double *stats, *runpart;
};

template <int K>
__global__ __launch_bounds__(256) void sparse_col_kernel(SpColArgs a) {
    using Cf = SpColCfg<K>;
    constexpr int GW = Cf::GW, NR = Cf::NR, NO = Cf::NO, EPL = Cf::EPL, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1), gbase = lane & ~(GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double *mu = a.model + MODEL_HDR + (int64_t)a.d * K;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double muj = mu[it.col];
        double acc[EPL];
#pragma unroll
        for (int p = 0; p < EPL; ++p) acc[p] = 0.0;
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group)
            const bool mine = t + sub < it.len;
            const int li = mine ? a.trow[it.start + t + sub] : 0;
            const double xv = mine ? a.tval[it.start + t + sub] - muj : 0.0;
            const int nb = it.len - t < GW ? it.len - t : GW;
            for (int q = 0; q < nb; q += 4) {  // the entries in ascending row, four record gathers in flight
                double x[4], v[4][EPL];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int src = gbase + ((q + u) & (GW - 1));
                    const int i = __shfl(li, src, 64);
                    x[u] = __shfl(xv, src, 64);
                    const bool ok = q + u < nb;  // (past the end: exact zeros, which change no sum)
                    const double *rr = a.rec + (int64_t)i * NR;
#pragma unroll
                    for (int p = 0; p < EPL; ++p) {
                        const int o = sub + p * GW;
                        v[u][p] = (ok && o < NO) ? rr[o < NR ? o : o - NR] : 0.0;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int p = 0; p < EPL; ++p) {
                        const int o = sub + p * GW;
                        acc[p] = o < NR ? acc[p] + v[u][p] : fma(x[u], v[u][p], acc[p]);
                    }
            }
        }
        if (live) {
#pragma unroll
            for (int p = 0; p < EPL; ++p) {
                const int o = sub + p * GW;
                if (o >= NO) continue;
                if (it.dest < 0) {
                    double *dst = a.stats + sp_stat_index(o, it.col, a.d, K);
                    *dst += acc[p];
                } else {
                    a.runpart[it.dest * NO + o] = acc[p];
                }
            }
        }
    }
}

// statistics of a long column += its runs' partials, added in run order
__global__ __launch_bounds__(256) void sparse_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, int k, double *stats) {
    const int no = sp_no(k);
    for (int64_t c = blockIdx.x; c < n_long; c += gridDim.x) {
        const SpLong lc = longs[c];
        for (int o = threadIdx.x; o < no; o += blockDim.x) {
            double s = 0.0;
            for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * no + o];
            stats[sp_stat_index(o, lc.col, d, k)] += s;
        }
    }
}

// query entries [q0, q1) (the query rows of one block): mean_j + c_j . z_i, c_j^T Sigma_i c_j + sigma^2
// (query_row's search and predict_entry's loop written out: called, they leave sigma^2 and the model's pointers inside the entry loop)
__global__ __launch_bounds__(256) void sparse_predict_kernel(const int64_t *qptr, const int32_t *qcol, int64_t q0, int64_t q1, int64_t row0,
                                                             int64_t rows, int d, int k, const double *model, const double *states,
                                                             const double *covs, double *mean, double *var) {
    const double *C = model + MODEL_HDR, *mu = C + (int64_t)d * k;
    const double s2 = model[1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < q1; e += stride) {
        int64_t lo = row0, hi = row0 + rows;  // the row r with qptr[r] <= e < qptr[r + 1]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (qptr[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        const int64_t lr = lo - row0;
        const int j = qcol[e];
        const double *c = C + (int64_t)j * k, *z = states + lr * k, *S = covs + lr * k * k;
        double dot = 0.0, q = 0.0;
        for (int t = 0; t < k; ++t) {
            dot = fma(c[t], z[t], dot);
            double sc = 0.0;
            for (int u = 0; u < k; ++u) sc = fma(S[t * k + u], c[u], sc);
            q = fma(c[t], sc, q);
        }
        mean[e] = mu[j] + dot;
        var[e] = q + s2;
    }
}

}  // namespace ppca_sp

namespace {

template <int K>
hipError_t row_t(const SpRowArgs &a, int grid, hipStream_t s) { return sp_launch(sparse_row_kernel<K>, grid, s, a); }
template <int K>
hipError_t col_t(const SpColArgs &a, int n_cu, hipStream_t s) {
    return sp_launch(sparse_col_kernel<K>, sp_grid(a.n_items, 4 * (64 / SpColCfg<K>::GW), n_cu, 8), s, a);
}
hipError_t launch_row(int k, const SpRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, row_t, a, grid, s); }
hipError_t launch_col(int k, const SpColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, col_t, a, n_cu, s); }

// ------------------------------------------------------------------ host: validation and the inverted index
int sp_validate(int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val) {
    if (n < 0 || d < 1 || !row_ptr) return fail(PPCA_ERR_INVALID, "bad shape or null row_ptr");
    if (row_ptr[0] != 0) return fail(PPCA_ERR_INVALID, "row_ptr must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(PPCA_ERR_INVALID, "row_ptr is not monotone at row %lld", (long long)i);
    const int64_t nnz = row_ptr[n];
    if (nnz > 0 && (!col || !val)) return fail(PPCA_ERR_INVALID, "null col or val");
    for (int64_t i = 0; i < n; ++i) {
        if (row_ptr[i + 1] - row_ptr[i] > d) return fail(PPCA_ERR_INVALID, "row %lld has more entries than columns", (long long)i);
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= d) return fail(PPCA_ERR_INVALID, "column %d of row %lld is outside [0, %d)", col[e], (long long)i, d);
            if (e > row_ptr[i] && col[e] <= col[e - 1])
                return fail(PPCA_ERR_INVALID, "columns of row %lld are not strictly increasing", (long long)i);
            if (!std::isfinite(val[e])) return fail(PPCA_ERR_INVALID, "value %lld of row %lld is not finite", (long long)(e - row_ptr[i]), (long long)i);
        }
    }
    return PPCA_OK;
}

// The inverted index of rows [r0, r1): a counting sort by column, stable in row order.  cp (d + 1): the column offsets, relative to
// the block's first entry; trow / tval: the block's slice of the outputs.
void sp_transpose_block(int64_t r0, int64_t r1, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val, int64_t *cp,
                        int64_t *cursor, int32_t *trow, double *tval) {
    std::fill(cp, cp + d + 1, (int64_t)0);
    const int64_t e0 = row_ptr[r0], e1 = row_ptr[r1];
    for (int64_t e = e0; e < e1; ++e) ++cp[col[e] + 1];
    for (int32_t j = 0; j < d; ++j) cp[j + 1] += cp[j];
    std::copy(cp, cp + d, cursor);
    for (int64_t i = r0; i < r1; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int64_t at = cursor[col[e]]++;
            trow[at] = (int32_t)(i - r0);
            tval[at] = val[e];
        }
}

int64_t sp_default_block_rows() { return ((int64_t)1 << 30) / (8 * (SP_MAX_K + 1 + SP_MAX_K * (SP_MAX_K + 1) / 2)); }

// scal8 (+)= the block's eight scalars; spart: ceil(max_rows / 1024) x 8 doubles of scratch
int sp_block_scalars(ppca_ctx *ctx, const SpBlock &b, const double *rscal, double *spart, double *scal8, int accumulate) {
    const int parts = (int)((b.rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS);
    HIP_TRY(sp_launch(sparse_scal_kernel, parts, ctx->stream, rscal, b.rows, spart));
    HIP_TRY(launch_reduce_partials(spart, parts, 8, scal8, ctx->stream, accumulate));
    return PPCA_OK;
}

}  // namespace

int ppca_sp::sp_upload(ppca_ctx *ctx, const void *src, size_t bytes, BufRef *out) {
    if (int rc = dev_alloc(std::max<size_t>(bytes, 8), out)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync((*out)->p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PPCA_OK;
}

int ppca_sp::sp_check(const ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model) {
    if (!ctx || !sp || !model) return fail(PPCA_ERR_INVALID, "null argument");
    if (sp->core->d != model->d)
        return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", sp->core->d, model->d);
    if (sp->ctx->device != model->ctx->device) return fail(PPCA_ERR_INVALID, "dataset and model live on different devices");
    if (model->k > SP_MAX_K)
        return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported on sparse data: the kernels cover k <= %d", model->k, SP_MAX_K);
    if (sp->core->n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    return PPCA_OK;
}

int ppca_sp::sp_rows_of_block(ppca_ctx *ctx, const ppca_sparse *sp, const SpBlock &b, const ppca_model *model, double *llks, double *states,
                              double *covs, double *rec, double *rscal) {
    SpRowArgs a{};
    a.w = sp->w;
    a.d = sp->core->d;
    a.model = model->p();
    a.llks = llks;
    a.states = states;
    a.covs = covs;
    a.rec = rec;
    a.rscal = rscal;
    const auto row = [&](const SpRowArgs &ba, int grid) { return launch_row(model->k, ba, grid, ctx->stream); };
    return sp_for_bins(ctx, sp, b, a, row);
}

int ppca_sp::sp_acc_scratch(const SpCore &c, int k, SpAccScratch *s) {
    const int nr = k + 1 + k * (k + 1) / 2;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * nr, &s->rec)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * SP_NSCAL, &s->rscal)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8 * (size_t)((c.max_rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS), &s->spart)) return rc;
    return dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * sp_no(k), &s->runpart);
}

int ppca_sp::sp_accumulate(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, double *stats, const SpAccScratch *scratch) {
    const SpCore &c = *sp->core;
    const int k = model->k;
    const StatsLayout L(c.d, k);
    SpAccScratch own;
    if (!scratch) {
        if (int rc = sp_acc_scratch(c, k, &own)) return rc;
        scratch = &own;
    }
    double *rec = dptr<double>(scratch->rec), *rscal = dptr<double>(scratch->rscal), *runpart = dptr<double>(scratch->runpart);
    HIP_TRY(hipMemsetAsync(stats, 0, sizeof(double) * (size_t)L.len, ctx->stream));
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_rows_of_block(ctx, sp, b, model, nullptr, nullptr, nullptr, rec, rscal)) return rc;
        if (int rc = sp_block_scalars(ctx, b, rscal, dptr<double>(scratch->spart), stats + L.scalars, 1)) return rc;
        SpColArgs a{};
        a.rec = rec;
        a.model = model->p();
        a.stats = stats;
        const auto item = [&](const SpColArgs &ba) { return launch_col(k, ba, ctx->n_cu, ctx->stream); };
        const auto fix = [&] {  // one workgroup per long column
            return sp_launch(sparse_fix_kernel, sp_grid(b.n_long, 1, ctx->n_cu, 8), ctx->stream, b.longs(), b.n_long, runpart, c.d, k, stats);
        };
        if (int rc = sp_col_pass(sp, b, runpart, a, item, fix)) return rc;
    }
    return PPCA_OK;
}

// ------------------------------------------------------------------ C-ABI
extern "C" int ppca_sparse_transpose_host(int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val,
                                          int64_t block_rows, int64_t *col_ptr_out, int32_t *t_row_out, double *t_val_out) {
    if (int rc = sp_validate(n, d, row_ptr, col, val)) return rc;
    if (block_rows < 0 || block_rows > INT32_MAX) return fail(PPCA_ERR_INVALID, "block_rows must lie in [0, 2^31)");
    if (row_ptr[n] > 0 && (!t_row_out || !t_val_out)) return fail(PPCA_ERR_INVALID, "null output");
    const int64_t br = block_rows > 0 ? block_rows : sp_default_block_rows();
    std::vector<int64_t> cp((size_t)d + 1), cursor((size_t)d);
    int64_t b = 0;
    for (int64_t r0 = 0; r0 < n; r0 += br, ++b) {
        const int64_t r1 = std::min(n, r0 + br), e0 = row_ptr[r0];
        sp_transpose_block(r0, r1, d, row_ptr, col, val, cp.data(), cursor.data(), t_row_out + e0, t_val_out + e0);
        if (col_ptr_out) std::copy(cp.begin(), cp.end(), col_ptr_out + b * ((int64_t)d + 1));
    }
    return PPCA_OK;
}

extern "C" int ppca_sparse_from_host(ppca_ctx *ctx, int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val,
                                     const double *weights, int64_t block_rows, int32_t segment, ppca_sparse **out) {
    if (!ctx || !out) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_validate(n, d, row_ptr, col, val)) return rc;
    if (block_rows < 0 || block_rows > INT32_MAX || segment < 0) return fail(PPCA_ERR_INVALID, "block_rows and segment must be >= 0");
    USE_CTX(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    auto core = std::make_shared<SpCore>();
    core->n = n;
    core->d = d;
    core->nnz = row_ptr[n];
    core->block_rows = block_rows > 0 ? block_rows : sp_default_block_rows();
    core->segment = segment > 0 ? segment : SP_SEGMENT;
    const int64_t nnz = core->nnz, seg = core->segment;
    std::vector<int32_t> trow((size_t)nnz);
    std::vector<double> tval((size_t)nnz);
    std::vector<int64_t> cp((size_t)d + 1), cursor((size_t)d);
    core->empty.assign((size_t)d, 1);
    struct HostBlock {
        std::vector<int32_t> rows;
        std::vector<SpItem> items;
        std::vector<SpLong> longs;
    };
    std::vector<HostBlock> hb;
    for (int64_t r0 = 0; r0 < n; r0 += core->block_rows) {
        const int64_t r1 = std::min(n, r0 + core->block_rows);
        SpBlock b;
        b.row0 = r0;
        b.rows = r1 - r0;
        b.e0 = row_ptr[r0];
        b.nnz = row_ptr[r1] - b.e0;
        if (b.nnz > INT32_MAX) return fail(PPCA_ERR_INVALID, "a block of %lld rows holds more than 2^31 entries: lower block_rows", (long long)b.rows);
        sp_transpose_block(r0, r1, d, row_ptr, col, val, cp.data(), cursor.data(), trow.data() + b.e0, tval.data() + b.e0);
        HostBlock h;
        for (int bin = 0; bin < 3; ++bin) {  // the row lists, each in ascending row
            b.bin_off[bin] = (int64_t)h.rows.size();
            for (int64_t i = r0; i < r1; ++i) {
                const int64_t m = row_ptr[i + 1] - row_ptr[i];
                const int which = m <= SP_SHORT ? 0 : m <= SP_MID ? 1 : 2;
                if (which == bin) h.rows.push_back((int32_t)(i - r0));
            }
            b.nbin[bin] = (int64_t)h.rows.size() - b.bin_off[bin];
        }
        for (int32_t j = 0; j < d; ++j) {
            const int64_t cnt = cp[j + 1] - cp[j];
            if (cnt == 0) continue;
            core->empty[j] = 0;
            if (cnt <= seg) {
                h.items.push_back(SpItem{b.e0 + cp[j], -1, j, (int32_t)cnt});
            } else {
                const int64_t nruns = (cnt + seg - 1) / seg;
                h.longs.push_back(SpLong{b.n_runs, j, (int32_t)nruns});
                for (int64_t r = 0; r < nruns; ++r)
                    h.items.push_back(SpItem{b.e0 + cp[j] + r * seg, b.n_runs + r, j, (int32_t)std::min(seg, cnt - r * seg)});
                b.n_runs += nruns;
            }
        }
        b.n_items = (int64_t)h.items.size();
        b.n_long = (int64_t)h.longs.size();
        core->max_rows = std::max(core->max_rows, b.rows);
        core->max_runs = std::max(core->max_runs, b.n_runs);
        core->blocks.push_back(b);
        hb.push_back(std::move(h));
    }
    for (int64_t i = 0; i < n; ++i) core->nonempty_rows += row_ptr[i + 1] > row_ptr[i] ? 1 : 0;
    core->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    auto sp = std::make_unique<ppca_sparse>();
    sp->ctx = ctx;
    int rc = PPCA_OK;
    do {
        if ((rc = sp_upload(ctx, row_ptr, sizeof(int64_t) * (size_t)(n + 1), &core->row_ptr_buf))) break;
        if ((rc = sp_upload(ctx, col, sizeof(int32_t) * (size_t)nnz, &core->col_buf))) break;
        if ((rc = sp_upload(ctx, val, sizeof(double) * (size_t)nnz, &core->val))) break;
        if ((rc = sp_upload(ctx, trow.data(), sizeof(int32_t) * (size_t)nnz, &core->trow_buf))) break;
        if ((rc = sp_upload(ctx, tval.data(), sizeof(double) * (size_t)nnz, &core->tval))) break;
        for (size_t i = 0; i < hb.size() && !rc; ++i) {
            SpBlock &b = core->blocks[i];
            if ((rc = sp_upload(ctx, hb[i].rows.data(), sizeof(int32_t) * hb[i].rows.size(), &b.rowlist_buf))) break;
            if ((rc = sp_upload(ctx, hb[i].items.data(), sizeof(SpItem) * hb[i].items.size(), &b.items_buf))) break;
            if ((rc = sp_upload(ctx, hb[i].longs.data(), sizeof(SpLong) * hb[i].longs.size(), &b.longs_buf))) break;
        }
        if (rc) break;
        if (weights) {
            if ((rc = sp_upload(ctx, weights, sizeof(double) * (size_t)n, &sp->wbuf))) break;
            sp->w = dptr<const double>(sp->wbuf);
        }
    } while (false);
    if ((rc = sp_finish(ctx, rc, "upload"))) return rc;  // the uploads read this call's host buffers
    sp->core = core;
    *out = sp.release();
    return PPCA_OK;
}

extern "C" int ppca_sparse_free(ppca_sparse *sp) {
    if (sp) {
        (void)hipSetDevice(sp->ctx->device);
        delete sp;
    }
    return PPCA_OK;
}
extern "C" int64_t ppca_sparse_len(const ppca_sparse *sp) { return sp ? sp->core->n : 0; }
extern "C" int32_t ppca_sparse_output_size(const ppca_sparse *sp) { return sp ? sp->core->d : 0; }
extern "C" int64_t ppca_sparse_nnz(const ppca_sparse *sp) { return sp ? sp->core->nnz : 0; }
extern "C" double ppca_sparse_build_seconds(const ppca_sparse *sp) { return sp ? sp->core->build_seconds : 0.0; }

extern "C" int ppca_sparse_with_weights(ppca_sparse *sp, const double *weights_host, ppca_sparse **out) {
    if (!sp || !out) return fail(PPCA_ERR_INVALID, "null argument");
    ppca_ctx *ctx = sp->ctx;
    USE_CTX(ctx);
    auto nd = std::make_unique<ppca_sparse>();
    nd->ctx = ctx;
    nd->core = sp->core;
    nd->vbuf = sp->vbuf;
    nd->tvbuf = sp->tvbuf;
    if (weights_host) {
        if (int rc = sp_upload(ctx, weights_host, sizeof(double) * (size_t)sp->core->n, &nd->wbuf)) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        nd->w = dptr<const double>(nd->wbuf);
    }
    *out = nd.release();
    return PPCA_OK;
}

extern "C" int ppca_sparse_to_host(ppca_sparse *sp, int64_t *row_ptr, int32_t *col, double *val, double *weights) {
    if (!sp) return fail(PPCA_ERR_INVALID, "null argument");
    ppca_ctx *ctx = sp->ctx;
    USE_CTX(ctx);
    const SpCore &c = *sp->core;
    if (row_ptr) HIP_TRY(hipMemcpyAsync(row_ptr, c.row_ptr(), sizeof(int64_t) * (size_t)(c.n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (col && c.nnz) HIP_TRY(hipMemcpyAsync(col, c.col(), sizeof(int32_t) * (size_t)c.nnz, hipMemcpyDeviceToHost, ctx->stream));
    if (val && c.nnz) HIP_TRY(hipMemcpyAsync(val, sp->val(), sizeof(double) * (size_t)c.nnz, hipMemcpyDeviceToHost, ctx->stream));
    if (weights && c.n) {
        if (sp->w)
            HIP_TRY(hipMemcpyAsync(weights, sp->w, sizeof(double) * (size_t)c.n, hipMemcpyDeviceToHost, ctx->stream));
        else
            std::fill(weights, weights + c.n, 1.0);
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PPCA_OK;
}

extern "C" int ppca_sparse_empty_dimensions(ppca_sparse *sp, int32_t *flags) {
    if (!sp || !flags) return fail(PPCA_ERR_INVALID, "null argument");
    std::copy(sp->core->empty.begin(), sp->core->empty.end(), flags);
    return PPCA_OK;
}

extern "C" int ppca_sparse_em_accumulate(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *stats_dev) {
    if (!stats_dev) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, sp, model)) return rc;
    USE_CTX(ctx);
    return sp_accumulate(ctx, sp, model, stats_dev);
}

extern "C" int ppca_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model_in, const ppca_prior *prior, ppca_model *out,
                                   double *llk_in) {
    if (!out) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, sp, model_in)) return rc;
    USE_CTX(ctx);
    const StatsLayout L(model_in->d, model_in->k);
    if (int rc = ensure(ctx->stats, ctx->stats_cap, sizeof(double) * (size_t)L.len)) return rc;
    double *stats = dptr<double>(ctx->stats);
    ctx->stats_llk_at = -1;
    if (int rc = sp_accumulate(ctx, sp, model_in, stats)) return rc;
    if (int rc = em_finalize_with_table(ctx, model_in, stats, prior, out)) return rc;
    ctx->stats_llk_at = L.scalars + SC_LLK;
    if (llk_in) {
        HIP_TRY(hipMemcpyAsync(llk_in, stats + L.scalars + SC_LLK, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return PPCA_OK;
}

extern "C" int ppca_sparse_stats_raw(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *stats_host) {
    if (!stats_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, sp, model)) return rc;
    USE_CTX(ctx);
    const StatsLayout L(model->d, model->k);
    if (int rc = ensure(ctx->stats, ctx->stats_cap, sizeof(double) * (size_t)L.len)) return rc;
    double *stats = dptr<double>(ctx->stats);
    ctx->stats_llk_at = -1;
    if (int rc = sp_accumulate(ctx, sp, model, stats)) return rc;
    HIP_TRY(hipMemcpyAsync(stats_host, stats, sizeof(double) * (size_t)L.len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PPCA_OK;
}

extern "C" int ppca_sparse_llk(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *total_host, double *per_row_host) {
    if (int rc = sp_check(ctx, sp, model)) return rc;
    USE_CTX(ctx);
    const SpCore &c = *sp->core;
    BufRef llks, rscal, spart, scal;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.n, &llks)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * SP_NSCAL, &rscal)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8 * (size_t)((c.max_rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS), &spart)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8, &scal)) return rc;
    HIP_TRY(hipMemsetAsync(scal->p, 0, sizeof(double) * 8, ctx->stream));
    double *rs = dptr<double>(rscal);
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_rows_of_block(ctx, sp, b, model, dptr<double>(llks) + b.row0, nullptr, nullptr, nullptr, rs)) return rc;
        if (int rc = sp_block_scalars(ctx, b, rs, dptr<double>(spart), dptr<double>(scal), 1)) return rc;
    }
    double h[8];
    HIP_TRY(hipMemcpyAsync(h, scal->p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    if (per_row_host) HIP_TRY(hipMemcpyAsync(per_row_host, llks->p, sizeof(double) * (size_t)c.n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (total_host) *total_host = h[SC_LLK];
    return PPCA_OK;
}

extern "C" int ppca_sparse_infer(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *states_host, double *covs_host) {
    if (int rc = sp_check(ctx, sp, model)) return rc;
    if (model->zero_state) return PPCA_OK;  // n x 0 states: nothing to write
    if (!states_host) return fail(PPCA_ERR_INVALID, "null argument");
    USE_CTX(ctx);
    const SpCore &c = *sp->core;
    const int k = model->k;
    BufRef st, cv;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k, &st)) return rc;
    if (covs_host)
        if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k * k, &cv)) return rc;
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_rows_of_block(ctx, sp, b, model, nullptr, dptr<double>(st), cv ? dptr<double>(cv) : nullptr, nullptr, nullptr)) return rc;
        HIP_TRY(hipMemcpyAsync(states_host + b.row0 * k, st->p, sizeof(double) * (size_t)b.rows * k, hipMemcpyDeviceToHost, ctx->stream));
        if (covs_host)
            HIP_TRY(hipMemcpyAsync(covs_host + b.row0 * k * k, cv->p, sizeof(double) * (size_t)b.rows * k * k, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the next block overwrites the scratch
    }
    return PPCA_OK;
}

int ppca_sp::sp_check_query(const SpCore &c, const int64_t *query_row_ptr, const int32_t *query_col, const double *mean_host,
                            const double *var_host, int64_t *nq) {
    if (!query_row_ptr) return fail(PPCA_ERR_INVALID, "null argument");
    if (query_row_ptr[0] != 0) return fail(PPCA_ERR_INVALID, "query row_ptr must start at 0");
    for (int64_t i = 0; i < c.n; ++i)
        if (query_row_ptr[i + 1] < query_row_ptr[i]) return fail(PPCA_ERR_INVALID, "query row_ptr is not monotone at row %lld", (long long)i);
    *nq = query_row_ptr[c.n];
    if (*nq == 0) return PPCA_OK;
    if (!query_col || !mean_host || !var_host) return fail(PPCA_ERR_INVALID, "null argument");
    for (int64_t e = 0; e < *nq; ++e)
        if (query_col[e] < 0 || query_col[e] >= c.d) return fail(PPCA_ERR_INVALID, "query column %d is outside [0, %d)", query_col[e], c.d);
    return PPCA_OK;
}

int ppca_sp::sp_predict(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, const int64_t *query_row_ptr, const int32_t *query_col,
                        double *mean_host, double *var_host, const SpRowPass &rows_of_block) {
    const SpCore &c = *sp->core;
    int64_t nq = 0;
    if (int rc = sp_check_query(c, query_row_ptr, query_col, mean_host, var_host, &nq)) return rc;
    if (nq == 0) return PPCA_OK;
    USE_CTX(ctx);
    const int k = model->k;
    BufRef st, cv, qp, qc, mean, var;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k, &st)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k * k, &cv)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &mean)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &var)) return rc;
    int rc = sp_upload(ctx, query_row_ptr, sizeof(int64_t) * (size_t)(c.n + 1), &qp);
    if (!rc) rc = sp_upload(ctx, query_col, sizeof(int32_t) * (size_t)nq, &qc);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        const int64_t q0 = query_row_ptr[b.row0], q1 = query_row_ptr[b.row0 + b.rows];
        if (q1 == q0) continue;
        rc = rows_of_block(b, dptr<double>(st), dptr<double>(cv));
        if (rc) break;
        if (sp_launch(sparse_predict_kernel, sp_elementwise_grid(q1 - q0, ctx->n_cu), ctx->stream, dptr<const int64_t>(qp), dptr<const int32_t>(qc), q0,
                      q1, b.row0, b.rows, c.d, k, model->p(), dptr<const double>(st), dptr<const double>(cv), dptr<double>(mean),
                      dptr<double>(var)))
            rc = fail(PPCA_ERR_HIP, "predict launch failed");
    }
    if (!rc && hipMemcpyAsync(mean_host, mean->p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(var_host, var->p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    return sp_finish(ctx, rc, "predict");  // (the uploads read the caller's buffers)
}

extern "C" int ppca_sparse_predict(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, const int64_t *query_row_ptr,
                                   const int32_t *query_col, double *mean_host, double *var_host) {
    if (int rc = sp_check(ctx, sp, model)) return rc;
    const auto rows = [&](const SpBlock &b, double *states, double *covs) {
        return sp_rows_of_block(ctx, sp, b, model, nullptr, states, covs, nullptr, nullptr);
    };
    return sp_predict(ctx, sp, model, query_row_ptr, query_col, mean_host, var_host, rows);
}
