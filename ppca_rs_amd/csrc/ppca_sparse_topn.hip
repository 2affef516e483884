// ppca_sparse_topn.hip -- top-n ranking on row-compressed data, for one model and for the mixture, which share the lists, the windows,
// the merge and the host helpers sp_top_*.  Storage and shared scaffolding: ppca_sparse.hpp.
//
// Top-n ranking (ppca_topn_sparse).  Per block: sparse_row_kernel<K> writes z (and Sigma when kappa != 0), then
// sparse_topn_kernel<K, VAR, R>  a wave takes a tile of R rows and a chunk of candidate positions and walks the chunk 64 at a time: a
//     lane holds c_j and mean_j of one column, z and Sigma of a row are wave-uniform, the score is sparse_predict_kernel's (mean, var)
//     multiply-add for multiply-add, and a row's list of n <= 64 (score, column) is held one entry per lane behind a wave-uniform
//     threshold.  The order (score descending, column ascending) is total, so the result depends on nothing else.
// sparse_topn_merge_kernel  when the columns were split into chunks: one wave per row offers the row's chunk lists in chunk order.
//
// The mixture's top-n ranking (ppca_mix_topn_sparse).  The posteriors once; per block sparse_mix_resp_kernel
// (r = exp(log posterior)), sparse_row_kernel<k_c> per component into one scratch in the layout of the largest state size
// (sparse_pad_kernel for a smaller component), then
// sparse_mix_topn_kernel<K, VAR, R>  sparse_topn_kernel's work items, lists and windows with a loop over the components per 64 columns:
//     the score is fma(kappa, sqrt(var), mean) with sparse_mix_predict_kernel / sparse_mix_spread_kernel's (mean, var), operation for
//     operation; sparse_topn_merge_kernel when the columns were split.
#include <climits>
#include <cmath>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

// ---- top-n ranking
constexpr int SP_TOP_MAX = 64;           // n_top: a row's list is held one entry per lane
constexpr int SP_TOP_R = 16;             // rows of a wave's tile when the score is the mean ...
constexpr int SP_TOP_RV = 4;             // ... and when it needs the variance (k^2 multiply-adds per score)
constexpr int SP_TOP_MINCHUNK = 1024;    // fewest candidate positions of a column chunk

struct SpTopDims {
    int64_t row0, rows;  // the block
    int d, nc;           // columns; candidate positions (d without a candidate list)
    int chunk, nchunks;  // candidate positions per column chunk (a multiple of 64)
    int n_top, exclude, final;
    double kappa;
};

// v of lane l (l uniform) as a wave-uniform value
__device__ __forceinline__ double lane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// A row's list, entry p on lane p (p < n): score descending, equal scores in ascending column; empty entries (-inf, -1) at the end;
// thr = the score of entry n - 1.  (s, j) goes in iff s > thr.  The callers offer columns in ascending order, so a score equal to a
// stored one goes behind it -- and one equal to thr stays out.
__device__ __forceinline__ void top_insert(double &ls, int &lc, double &thr, double s, int j, int lane, int n) {
    if (!(s > thr)) return;  // (uniform)
    const int p = __popcll(__ballot(ls >= s));
    const double us = __shfl_up(ls, 1, 64);
    const int uc = __shfl_up(lc, 1, 64);
    if (lane == p) {
        ls = s;
        lc = j;
    } else if (lane > p && lane < n) {
        ls = us;
        lc = uc;
    }
    thr = lane_f64(ls, n - 1);
}

// The row's own columns, for exclude_observed: a window of 64 of its m sorted CSR columns is kept in a register, lane l of rc =
// col[e0 + w + l] (INT_MAX past the row's end), w a multiple of 64.  Columns are offered in ascending order, so the window only moves
// forward: a row of at most 64 entries is read once per work item, a longer one at most m / 64 times.
__device__ __forceinline__ int top_window(const int32_t *col, int64_t e0, int m, int w, int lane) {
    return w + lane < m ? col[e0 + w + lane] : INT_MAX;
}
// the window a chunk that starts at column jstart begins with: the last one whose first column is <= jstart (uniform)
__device__ __forceinline__ int top_window_start(const int32_t *col, int64_t e0, int m, int jstart) {
    int lo = 0, hi = (m - 1) / 64;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (col[e0 + (int64_t)mid * 64] <= jstart)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo * 64;
}

// The lanes flagged in `beat` hold a score above the row's threshold (their columns span [jlo, jhi]): drop the columns the row has
// an entry in, then insert the others in ascending lane = ascending column.
__device__ __forceinline__ void top_offer(double &ls, int &lc, double &thr, bool beat, double score, int j, bool exclude, int &rc, int &w,
                                          const int32_t *col, int64_t e0, int m, int lane, int n) {
    uint64_t bm = __ballot(beat);
    if (exclude) {
        const int jlo = __builtin_amdgcn_readlane(j, __builtin_ctzll(bm)), jhi = __builtin_amdgcn_readlane(j, 63 - __builtin_clzll(bm));
        bool obs = false;
        for (;;) {  // (uniform)
            uint64_t in = __ballot(rc >= jlo && rc <= jhi);
            while (in) {
                obs |= j == __builtin_amdgcn_readlane(rc, __builtin_ctzll(in));
                in &= in - 1;
            }
            if (w + 64 >= m || __builtin_amdgcn_readlane(rc, 63) > jhi) break;
            w += 64;
            rc = top_window(col, e0, m, w, lane);
        }
        bm = __ballot(beat && !obs);
    }
    while (bm) {  // (uniform)
        const int l = __builtin_ctzll(bm);
        bm &= bm - 1;
        top_insert(ls, lc, thr, lane_f64(score, l), __builtin_amdgcn_readlane(j, l), lane, n);
    }
}

// A work item = (tile of R rows, column chunk), one wave each; tiles vary fastest, so the waves of a workgroup read the same rows of C.
// Lane l holds c_j and mean_j of candidate position base + l for the whole tile; z (and Sigma) of a row are wave-uniform operands.
// mean and var are sparse_predict_kernel's expressions, multiply-add for multiply-add.  Output: the item's list per row, at
// [(row * nchunks + chunk) * n_top + p]; with one chunk that is the result (empty entries as -1 / NaN).
template <int K, bool VAR, int R>
__global__ __launch_bounds__(256) void sparse_topn_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                          const int32_t *__restrict__ cand, const double *__restrict__ model,
                                                          const double *__restrict__ states, const double *__restrict__ covs,
                                                          double *__restrict__ ps, int32_t *__restrict__ pc, SpTopDims g) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = g.n_top;
    const int64_t ntiles = (g.rows + R - 1) / R, nitems = ntiles * g.nchunks;
    const double s2 = model[1];
    const double *C = model + MODEL_HDR, *mu = C + (int64_t)g.d * K;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wid; item < nitems; item += (int64_t)gridDim.x * 4) {  // (uniform over the wave)
        const int ch = (int)(item / ntiles);
        const int64_t r0 = (item % ntiles) * R;
        const int nr = (int)(g.rows - r0 < R ? g.rows - r0 : R);
        double ls[R], thr[R];
        int lc[R], rc[R], win[R];  // (rc, win: the window of each row's own columns, for exclude_observed)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ls[r] = -INFINITY;
            thr[r] = -INFINITY;
            lc[r] = -1;
            rc[r] = INT_MAX;
            win[r] = 0;
        }
        const int64_t p0 = (int64_t)ch * g.chunk, p1 = p0 + g.chunk < g.nc ? p0 + g.chunk : g.nc;
        if (g.exclude && p0 < p1) {
            const int jstart = cand ? cand[p0] : (int)p0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;  // (uniform)
                const int64_t row = g.row0 + r0 + r, e0 = row_ptr[row];
                const int m = (int)(row_ptr[row + 1] - e0);
                win[r] = (m > 64 && p0 > 0) ? top_window_start(col, e0, m, jstart) : 0;
                rc[r] = top_window(col, e0, m, win[r], lane);
            }
        }
        // the tile after the one being ranked is loaded while that one is ranked
        auto load = [&](int64_t base, bool &valid, int &j, double *c, double &muj) {
            const int64_t idx = base + lane;
            valid = idx < p1;
            j = valid ? (cand ? cand[idx] : (int)idx) : 0;
            const double *cj = C + (int64_t)j * K;
#pragma unroll
            for (int t = 0; t < K; ++t) c[t] = cj[t];
            muj = mu[j];
        };
        bool valid, nvalid = false;
        int j, nj = 0;
        double c[K], ncv[K], muj, nmuj = 0.0;
        if (p0 < p1) load(p0, valid, j, c, muj);
        for (int64_t base = p0; base < p1; base += 64) {
            if (base + 64 < p1) load(base + 64, nvalid, nj, ncv, nmuj);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;  // (uniform)
                const double *z = states + (r0 + r) * K;
                double dot = 0.0, q = 0.0;
#pragma unroll
                for (int t = 0; t < K; ++t) dot = fma(c[t], z[t], dot);
                double score = muj + dot;
                if (VAR) {
                    const double *S = covs + (r0 + r) * (K * K);
#pragma unroll
                    for (int t = 0; t < K; ++t) {
                        double sc = 0.0;
#pragma unroll
                        for (int u = 0; u < K; ++u) sc = fma(S[t * K + u], c[u], sc);
                        q = fma(c[t], sc, q);
                    }
                    score = fma(g.kappa, sqrt(q + s2), score);
                }
                const bool beat = valid && score > thr[r];
                if (__ballot(beat)) {
                    const int64_t row = g.row0 + r0 + r, e0 = row_ptr[row];
                    top_offer(ls[r], lc[r], thr[r], beat, score, j, g.exclude != 0, rc[r], win[r], col, e0, (int)(row_ptr[row + 1] - e0), lane, n);
                }
            }
            valid = nvalid;
            j = nj;
            muj = nmuj;
#pragma unroll
            for (int t = 0; t < K; ++t) c[t] = ncv[t];
        }
        if (lane < n) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;
                const int64_t at = ((r0 + r) * g.nchunks + ch) * n + lane;
                ps[at] = (g.final && lc[r] < 0) ? (double)NAN : ls[r];
                pc[at] = lc[r];
            }
        }
    }
}

// One wave per row: the row's chunk lists, offered in chunk order (ascending columns) entry by entry.
__global__ __launch_bounds__(256) void sparse_topn_merge_kernel(const double *__restrict__ ps, const int32_t *__restrict__ pc, int64_t rows,
                                                                int nchunks, int n, double *__restrict__ os, int32_t *__restrict__ oc) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wid; row < rows; row += (int64_t)gridDim.x * 4) {  // (uniform over the wave)
        double ls = -INFINITY, thr = -INFINITY;
        int lc = -1;
        for (int ch = 0; ch < nchunks; ++ch) {
            const int64_t at = (row * nchunks + ch) * n + lane;
            const double s = lane < n ? ps[at] : -INFINITY;
            const int j = lane < n ? pc[at] : -1;
            for (int p = 0; p < n; ++p) {
                const double sp = lane_f64(s, p);
                if (!(sp > thr)) break;  // (uniform; the list is sorted: nothing behind it gets in either)
                top_insert(ls, lc, thr, sp, __builtin_amdgcn_readlane(j, p), lane, n);
            }
        }
        if (lane < n) {
            os[row * n + lane] = lc < 0 ? (double)NAN : ls;
            oc[row * n + lane] = lc;
        }
    }
}

// ---- the mixture's top-n ranking
struct SpMixComp {    // a component as sparse_mix_topn_kernel<K, ..> reads it
    const double *C;  // d x K: the component's own C, or its copy with the rows zero-padded from k_c to K
    const double *mu;
    const double *model;  // sigma^2 at [1]
};

// dst (rows x kout, or rows x kout x kout with `square`) = src (rows x kin, or rows x kin x kin) with zeros behind: a component of
// a smaller state size in the layout of the largest (a trailing zero term leaves an fma chain that started at +0 as it was)
__global__ __launch_bounds__(256) void sparse_pad_kernel(const double *__restrict__ src, int64_t rows, int kin, int kout, int square,
                                                         double *__restrict__ dst) {
    const int64_t per = square ? (int64_t)kout * kout : kout, pin = square ? (int64_t)kin * kin : kin, len = rows * per;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
        const int64_t row = i / per;
        const int e = (int)(i - row * per), t = square ? e / kout : 0, u = square ? e % kout : e;
        dst[i] = (t < kin && u < kin) ? src[row * pin + (square ? t * kin + u : u)] : 0.0;
    }
}

// r[i] = exp(logpost[i]): the factor of sparse_mix_predict_kernel / sparse_mix_spread_kernel, once per (row, component)
__global__ __launch_bounds__(256) void sparse_mix_resp_kernel(const double *__restrict__ logpost, int64_t len, double *__restrict__ r) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) r[i] = exp(logpost[i]);
}

// The mixture's combination, in the operations of sparse_mix_predict_kernel and sparse_mix_spread_kernel.  There the steps are
// separated by stores and loads; here they meet in one kernel, where the compiler would contract across them (r0 v0 + s into one
// fused operation at one component, for one).  So: no contraction in these three, and the multiply-adds of those kernels as fma.
__device__ __forceinline__ void mix_top_add(bool first, double r, double m, double v, bool with_var, double &mean, double &var) {
#pragma clang fp contract(off)
    mean = first ? r * m : fma(r, m, mean);
    if (with_var) var = first ? r * v : fma(r, v, var);
}
__device__ __forceinline__ double mix_top_spread(double r, double m, double mean, double s) {
#pragma clang fp contract(off)
    const double dv = m - mean;
    return fma(r, dv * dv, s);
}
__device__ __forceinline__ double mix_top_score(double kappa, double var, double s, double mean) {
#pragma clang fp contract(off)
    const double total = var + s;
    return fma(kappa, sqrt(total), mean);
}

// sparse_topn_kernel for the mixture: the same work items, tile walk, lists and windows; per 64 candidate positions the wave loops
// over the components.  Lane l holds c_j and mean_j of ONE component at a time (the next component's, or the next tile's first, is
// loaded while this one is used); z, Sigma (scratch of all components: component c's rows at c * cap) and r of a row are
// wave-uniform operands.  (m_c, v_c) are predict_entry's, multiply-add for multiply-add, at the largest state size K: a smaller
// component is zero-padded (sparse_pad_kernel).  mean[R] and var[R] add the components in index order.  With VAR the spread needs
// every m_c again once the mean is final: a second loop over the components recomputes it (K multiply-adds beside the K^2 + 2 K of
// the first: no m_c is kept, so nm is not bounded by registers or LDS).
// floor = -inf, the threshold of an empty list, is an argument, not a literal: from K = 13 on the compiler holds the R = 16 thresholds
// in scalar registers that it fills with one 64-bit move each, and the move's 32-bit literal field keeps the low half of the
// constant -- 0, so columns with a score below 0.0 never reached a list that was not yet full.
template <int K, bool VAR, int R>
__global__ __launch_bounds__(256) void sparse_mix_topn_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ cand, const SpMixComp *__restrict__ comps,
                                                              const double *__restrict__ resp, const double *__restrict__ states,
                                                              const double *__restrict__ covs, double *__restrict__ ps,
                                                              int32_t *__restrict__ pc, SpTopDims g, int nm, int64_t cap, double floor) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n = g.n_top;
    const int64_t ntiles = (g.rows + R - 1) / R, nitems = ntiles * g.nchunks;
    const int nsteps = VAR ? 2 * nm : nm;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wid; item < nitems; item += (int64_t)gridDim.x * 4) {  // (uniform over the wave)
        const int ch = (int)(item / ntiles);
        const int64_t r0 = (item % ntiles) * R;
        const int nr = (int)(g.rows - r0 < R ? g.rows - r0 : R);
        double ls[R], thr[R];
        int lc[R], rc[R], win[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ls[r] = -INFINITY;
            thr[r] = floor;
            lc[r] = -1;
            rc[r] = INT_MAX;
            win[r] = 0;
        }
        const int64_t p0 = (int64_t)ch * g.chunk, p1 = p0 + g.chunk < g.nc ? p0 + g.chunk : g.nc;
        if (g.exclude && p0 < p1) {
            const int jstart = cand ? cand[p0] : (int)p0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;  // (uniform)
                const int64_t row = g.row0 + r0 + r, e0 = row_ptr[row];
                const int m = (int)(row_ptr[row + 1] - e0);
                win[r] = (m > 64 && p0 > 0) ? top_window_start(col, e0, m, jstart) : 0;
                rc[r] = top_window(col, e0, m, win[r], lane);
            }
        }
        auto column = [&](int64_t base, bool &valid, int &j) {
            const int64_t idx = base + lane;
            valid = idx < p1;
            j = valid ? (cand ? cand[idx] : (int)idx) : 0;
        };
        auto load = [&](int j, int comp, double *c, double &muj) {
            const double *cj = comps[comp].C + (int64_t)j * K;
#pragma unroll
            for (int t = 0; t < K; ++t) c[t] = cj[t];
            muj = comps[comp].mu[j];
        };
        bool valid = false, nvalid = false;
        int j = 0, nj = 0;
        double c[K], ncv[K], muj = 0.0, nmuj = 0.0;
        if (p0 < p1) {
            column(p0, valid, j);
            load(j, 0, c, muj);
        }
        for (int64_t base = p0; base < p1; base += 64) {
            const bool more = base + 64 < p1;
            if (more) column(base + 64, nvalid, nj);
            double mean[R], var[R], spread[R];
#pragma unroll
            for (int r = 0; r < R; ++r) mean[r] = var[r] = spread[r] = 0.0;
#pragma unroll 1
            for (int step = 0; step < nsteps; ++step) {  // (uniform) the components, then -- VAR -- the components again
                const bool again = step >= nm;
                const int comp = again ? step - nm : step;
                if (step + 1 < nsteps)
                    load(j, step + 1 >= nm ? step + 1 - nm : step + 1, ncv, nmuj);
                else if (more)
                    load(nj, 0, ncv, nmuj);
                const double s2 = comps[comp].model[1];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r >= nr) continue;  // (uniform)
                    const int64_t at = (int64_t)comp * cap + r0 + r;
                    const double *z = states + at * K;
                    const double w = resp[(r0 + r) * nm + comp];
                    double dot = 0.0;
#pragma unroll
                    for (int t = 0; t < K; ++t) dot = fma(c[t], z[t], dot);
                    const double m = muj + dot;
                    if (VAR && again) {
                        spread[r] = mix_top_spread(w, m, mean[r], spread[r]);
                        continue;
                    }
                    double v = 0.0;
                    if (VAR) {
                        const double *S = covs + at * (K * K);
                        double q = 0.0;
#pragma unroll
                        for (int t = 0; t < K; ++t) {
                            double sc = 0.0;
#pragma unroll
                            for (int u = 0; u < K; ++u) sc = fma(S[t * K + u], c[u], sc);
                            q = fma(c[t], sc, q);
                        }
                        v = q + s2;
                    }
                    mix_top_add(comp == 0, w, m, v, VAR, mean[r], var[r]);
                }
                muj = nmuj;
#pragma unroll
                for (int t = 0; t < K; ++t) c[t] = ncv[t];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;  // (uniform)
                const double score = VAR ? mix_top_score(g.kappa, var[r], spread[r], mean[r]) : mean[r];
                const bool beat = valid && score > thr[r];
                if (__ballot(beat)) {
                    const int64_t row = g.row0 + r0 + r, e0 = row_ptr[row];
                    top_offer(ls[r], lc[r], thr[r], beat, score, j, g.exclude != 0, rc[r], win[r], col, e0, (int)(row_ptr[row + 1] - e0), lane, n);
                }
            }
            valid = nvalid;
            j = nj;
        }
        if (lane < n) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r >= nr) continue;
                const int64_t at = ((r0 + r) * g.nchunks + ch) * n + lane;
                ps[at] = (g.final && lc[r] < 0) ? (double)NAN : ls[r];
                pc[at] = lc[r];
            }
        }
    }
}

}  // namespace ppca_sp

namespace {

struct SpTopPtrs {
    const int64_t *row_ptr;
    const int32_t *col, *cand;
    const double *model, *states, *covs;
    double *ps;
    int32_t *pc;
};
inline int64_t sp_top_tiles(int64_t rows, bool var) {
    const int r = var ? SP_TOP_RV : SP_TOP_R;
    return (rows + r - 1) / r;
}
template <int K>
hipError_t topn_t(const SpTopPtrs &p, const SpTopDims &g, bool var, int n_cu, hipStream_t s) {
    const int grid = sp_grid(sp_top_tiles(g.rows, var) * g.nchunks, 4, n_cu, 8);
    const auto kernel = var ? sparse_topn_kernel<K, true, SP_TOP_RV> : sparse_topn_kernel<K, false, SP_TOP_R>;
    return sp_launch(kernel, grid, s, p.row_ptr, p.col, p.cand, p.model, p.states, p.covs, p.ps, p.pc, g);
}
hipError_t launch_topn(int k, const SpTopPtrs &p, const SpTopDims &g, bool var, int n_cu, hipStream_t s) { SP_DISPATCH(k, topn_t, p, g, var, n_cu, s); }
struct SpMixTopPtrs {
    const int64_t *row_ptr;
    const int32_t *col, *cand;
    const SpMixComp *comps;
    const double *resp, *states, *covs;
    double *ps;
    int32_t *pc;
    int nm;
    int64_t cap;  // rows of a component's slice of states / covs
};
template <int K>
hipError_t mix_topn_t(const SpMixTopPtrs &p, const SpTopDims &g, bool var, int n_cu, hipStream_t s) {
    const int grid = sp_grid(sp_top_tiles(g.rows, var) * g.nchunks, 4, n_cu, 8);
    const auto kernel = var ? sparse_mix_topn_kernel<K, true, SP_TOP_RV> : sparse_mix_topn_kernel<K, false, SP_TOP_R>;
    return sp_launch(kernel, grid, s, p.row_ptr, p.col, p.cand, p.comps, p.resp, p.states, p.covs, p.ps, p.pc, g, p.nm, p.cap, -(double)INFINITY);
}
hipError_t launch_mix_topn(int k, const SpMixTopPtrs &p, const SpTopDims &g, bool var, int n_cu, hipStream_t s) {
    SP_DISPATCH(k, mix_topn_t, p, g, var, n_cu, s);
}

// the arguments that ppca_topn_sparse and ppca_mix_topn_sparse share, in the order their checks are documented
int sp_top_check(const SpCore &c, int32_t n_top, double kappa, const int32_t *candidates, int64_t n_candidates, const int32_t *cols_host,
                 const double *scores_host) {
    if (n_top < 1 || n_top > SP_TOP_MAX) return fail(PPCA_ERR_INVALID, "n_top = %d is outside [1, %d]", n_top, SP_TOP_MAX);
    if (!std::isfinite(kappa)) return fail(PPCA_ERR_INVALID, "kappa must be finite");
    if (!cols_host || !scores_host) return fail(PPCA_ERR_INVALID, "null output");
    if (n_candidates < 0 || n_candidates > c.d) return fail(PPCA_ERR_INVALID, "n_candidates = %lld is outside [0, %d]", (long long)n_candidates, c.d);
    if (candidates)
        for (int64_t i = 0; i < n_candidates; ++i) {
            if (candidates[i] < 0 || candidates[i] >= c.d) return fail(PPCA_ERR_INVALID, "candidate column %d is outside [0, %d)", candidates[i], c.d);
            if (i > 0 && candidates[i] <= candidates[i - 1]) return fail(PPCA_ERR_INVALID, "candidate columns are not strictly increasing at %lld", (long long)i);
        }
    return PPCA_OK;
}

// the column split: chunks so that (row tiles) x (chunks) fills the device, none under SP_TOP_MINCHUNK positions.  The order of the
// list is total, so the result does not depend on this choice.
int sp_top_chunks(int n_cu, int64_t rows, bool var, int nc, int *chunk) {
    const int64_t target = (int64_t)std::max(n_cu, 1) * 32;
    int64_t nch = std::max<int64_t>(1, std::min<int64_t>(target / sp_top_tiles(rows, var), nc / SP_TOP_MINCHUNK));
    const int64_t per = std::max<int64_t>(64, ((nc + nch - 1) / nch + 63) / 64 * 64);
    *chunk = (int)per;
    return (int)std::max<int64_t>(1, (nc + per - 1) / per);
}

// the result and scratch of a top-n call: one block's lists and, where a block's columns are split, its chunk lists
struct SpTopOut {
    BufRef os, oc, ps, pc;
};
int sp_top_out(const ppca_ctx *ctx, const SpCore &c, int n_top, bool var, int nc, SpTopOut *o) {
    int64_t part_len = 0;
    for (const SpBlock &b : c.blocks) {
        int chunk;
        const int nch = sp_top_chunks(ctx->n_cu, b.rows, var, nc, &chunk);
        if (nch > 1) part_len = std::max(part_len, b.rows * nch * n_top);
    }
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * n_top, &o->os)) return rc;
    if (int rc = dev_alloc(sizeof(int32_t) * (size_t)c.max_rows * n_top, &o->oc)) return rc;
    if (part_len > 0) {
        if (int rc = dev_alloc(sizeof(double) * (size_t)part_len, &o->ps)) return rc;
        if (int rc = dev_alloc(sizeof(int32_t) * (size_t)part_len, &o->pc)) return rc;
    }
    return PPCA_OK;
}
SpTopDims sp_top_dims(const ppca_ctx *ctx, const SpCore &c, const SpBlock &b, int n_top, double kappa, int exclude_observed, int nc) {
    SpTopDims g{};
    g.row0 = b.row0;
    g.rows = b.rows;
    g.d = c.d;
    g.nc = nc;
    g.nchunks = sp_top_chunks(ctx->n_cu, b.rows, kappa != 0.0, nc, &g.chunk);
    g.n_top = n_top;
    g.exclude = exclude_observed ? 1 : 0;
    g.final = g.nchunks == 1;
    g.kappa = kappa;
    return g;
}
// behind a block's ranking kernel: the merge of its chunk lists where the columns were split, then the block's rows of the result
int sp_top_finish(ppca_ctx *ctx, const SpBlock &b, const SpTopDims &g, const SpTopOut &o, int32_t *cols_host, double *scores_host) {
    const int n_top = g.n_top;
    if (!g.final) {
        if (sp_launch(sparse_topn_merge_kernel, sp_grid(b.rows, 4, ctx->n_cu, 8), ctx->stream, dptr<const double>(o.ps), dptr<const int32_t>(o.pc), b.rows,
                      g.nchunks, n_top, dptr<double>(o.os), dptr<int32_t>(o.oc)))
            return fail(PPCA_ERR_HIP, "top-n merge launch failed");
    }
    if (hipMemcpyAsync(scores_host + b.row0 * n_top, o.os->p, sizeof(double) * (size_t)b.rows * n_top, hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipMemcpyAsync(cols_host + b.row0 * n_top, o.oc->p, sizeof(int32_t) * (size_t)b.rows * n_top, hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)  // (the next block overwrites the scratch)
        return fail(PPCA_ERR_HIP, "top-n failed: %s", hipGetErrorString(hipGetLastError()));
    return PPCA_OK;
}
// what both ranking kernels read: the CSR pattern, the candidate list and the lists they write (the result, or the chunk lists)
template <class Ptrs>
void sp_top_ptrs(Ptrs &p, const SpCore &c, const BufRef &cand, const SpTopDims &g, const SpTopOut &o) {
    p.row_ptr = c.row_ptr();
    p.col = c.col();
    p.cand = cand ? dptr<const int32_t>(cand) : nullptr;
    p.ps = dptr<double>(g.final ? o.os : o.ps);
    p.pc = dptr<int32_t>(g.final ? o.oc : o.pc);
}

}  // namespace

extern "C" int ppca_topn_sparse(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, int32_t n_top, double kappa, int32_t exclude_observed,
                                const int32_t *candidates, int64_t n_candidates, int32_t *cols_host, double *scores_host) {
    if (int rc = sp_check(ctx, sp, model)) return rc;
    const SpCore &c = *sp->core;
    if (int rc = sp_top_check(c, n_top, kappa, candidates, n_candidates, cols_host, scores_host)) return rc;
    USE_CTX(ctx);
    const int k = model->k, nc = candidates ? (int)n_candidates : c.d;
    const bool var = kappa != 0.0;
    BufRef st, cv, cd;
    SpTopOut o;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k, &st)) return rc;
    if (var)
        if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * k * k, &cv)) return rc;
    if (int rc = sp_top_out(ctx, c, n_top, var, nc, &o)) return rc;
    int rc = PPCA_OK;
    if (candidates) rc = sp_upload(ctx, candidates, sizeof(int32_t) * (size_t)n_candidates, &cd);
    double *stp = dptr<double>(st), *cvp = var ? dptr<double>(cv) : nullptr;
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        rc = sp_rows_of_block(ctx, sp, b, model, nullptr, stp, cvp, nullptr, nullptr);
        if (rc) break;
        const SpTopDims g = sp_top_dims(ctx, c, b, n_top, kappa, exclude_observed, nc);
        SpTopPtrs p{};
        sp_top_ptrs(p, c, cd, g, o);
        p.model = model->p();
        p.states = stp;
        p.covs = cvp;
        if (launch_topn(k, p, g, var, ctx->n_cu, ctx->stream) != hipSuccess) {
            rc = fail(PPCA_ERR_HIP, "top-n launch failed");
            break;
        }
        rc = sp_top_finish(ctx, b, g, o, cols_host, scores_host);
    }
    return sp_finish(ctx, rc, "top-n");  // (the upload reads the caller's buffer)
}

// The mixture's: the posteriors once, then per block r = exp(log posterior), every component's row pass into
// ONE scratch (component c's rows at c * max_rows, in the layout of the largest state size K), sparse_mix_topn_kernel<K, ..>, and the
// merge and download of ppca_topn_sparse.
extern "C" int ppca_mix_topn_sparse(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                                    int32_t n_top, double kappa, int32_t exclude_observed, const int32_t *candidates, int64_t n_candidates,
                                    int32_t *cols_host, double *scores_host) {
    if (int rc = sp_mix_check(ctx, sp, models, log_weights, n_models)) return rc;
    const SpCore &c = *sp->core;
    if (int rc = sp_top_check(c, n_top, kappa, candidates, n_candidates, cols_host, scores_host)) return rc;
    USE_CTX(ctx);
    const int nm = n_models, nc = candidates ? (int)n_candidates : c.d;
    const bool var = kappa != 0.0;
    int K = 1, ksmall = 0;  // the largest state size, and the largest below it (0: the components agree)
    for (int e = 0; e < nm; ++e) K = std::max(K, models[e]->k);
    for (int e = 0; e < nm; ++e)
        if (models[e]->k < K) ksmall = std::max(ksmall, models[e]->k);
    const size_t cap = (size_t)c.max_rows;
    // every device block of the call, before its first launch
    SpMixDev m;
    if (int rc = sp_mix_blocks(ctx, c.n, nm, true, &m)) return rc;
    BufRef st, cv, tst, tcv, resp, cd, table;
    std::vector<BufRef> padded((size_t)nm);
    SpTopOut o;
    if (int rc = dev_alloc(sizeof(double) * cap * nm * K, &st)) return rc;
    if (var)
        if (int rc = dev_alloc(sizeof(double) * cap * nm * K * K, &cv)) return rc;
    if (ksmall > 0) {  // a smaller component's row pass writes its own layout here; sparse_pad_kernel moves it
        if (int rc = dev_alloc(sizeof(double) * cap * ksmall, &tst)) return rc;
        if (var)
            if (int rc = dev_alloc(sizeof(double) * cap * ksmall * ksmall, &tcv)) return rc;
    }
    if (int rc = dev_alloc(sizeof(double) * cap * nm, &resp)) return rc;
    if (int rc = dev_alloc(sizeof(SpMixComp) * (size_t)nm, &table)) return rc;
    for (int e = 0; e < nm; ++e)
        if (models[e]->k < K)
            if (int rc = dev_alloc(sizeof(double) * (size_t)c.d * K, &padded[e])) return rc;
    if (int rc = sp_top_out(ctx, c, n_top, var, nc, &o)) return rc;
    std::vector<SpMixComp> comps((size_t)nm);  // (read by the upload: alive until the synchronisation below)
    int rc = PPCA_OK;
    for (int e = 0; e < nm && !rc; ++e) {
        const int ke = models[e]->k;
        const double *mp = models[e]->p();
        comps[e].C = mp + MODEL_HDR;
        comps[e].mu = mp + MODEL_HDR + (int64_t)c.d * ke;
        comps[e].model = mp;
        if (ke < K) {
            double *pd = dptr<double>(padded[e]);
            if (sp_launch(sparse_pad_kernel, sp_elementwise_grid((int64_t)c.d * K, ctx->n_cu), ctx->stream, comps[e].C, (int64_t)c.d, ke, K, 0, pd))
                rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
            comps[e].C = pd;
        }
    }
    SpMixComp *table_dev = dptr<SpMixComp>(table);
    if (!rc && hipMemcpyAsync(table_dev, comps.data(), sizeof(SpMixComp) * (size_t)nm, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "upload failed");
    if (!rc && candidates) rc = sp_upload(ctx, candidates, sizeof(int32_t) * (size_t)n_candidates, &cd);
    if (!rc) rc = sp_mix_posteriors(ctx, sp, models, log_weights, nm, m);
    double *stp = dptr<double>(st), *cvp = var ? dptr<double>(cv) : nullptr, *rp = dptr<double>(resp);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        if (sp_launch(sparse_mix_resp_kernel, sp_elementwise_grid(b.rows * nm, ctx->n_cu), ctx->stream, m.logpost + b.row0 * nm, b.rows * nm, rp))
            rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
        for (int e = 0; e < nm && !rc; ++e) {
            const int ke = models[e]->k;
            double *zs = stp + cap * e * K, *ss = var ? cvp + cap * e * K * K : nullptr;
            if (ke == K) {
                rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, zs, ss, nullptr, nullptr);
                continue;
            }
            double *tz = dptr<double>(tst), *ts = var ? dptr<double>(tcv) : nullptr;
            rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, tz, ts, nullptr, nullptr);
            if (rc) break;
            hipError_t pe = sp_launch(sparse_pad_kernel, sp_elementwise_grid(b.rows * K, ctx->n_cu), ctx->stream, tz, b.rows, ke, K, 0, zs);
            if (var && !pe) pe = sp_launch(sparse_pad_kernel, sp_elementwise_grid(b.rows * K * K, ctx->n_cu), ctx->stream, ts, b.rows, ke, K, 1, ss);
            if (pe) rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
        }
        if (rc) break;
        const SpTopDims g = sp_top_dims(ctx, c, b, n_top, kappa, exclude_observed, nc);
        SpMixTopPtrs p{};
        sp_top_ptrs(p, c, cd, g, o);
        p.comps = table_dev;
        p.resp = rp;
        p.states = stp;
        p.covs = cvp;
        p.nm = nm;
        p.cap = (int64_t)cap;
        if (launch_mix_topn(K, p, g, var, ctx->n_cu, ctx->stream) != hipSuccess) {
            rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
            break;
        }
        rc = sp_top_finish(ctx, b, g, o, cols_host, scores_host);
    }
    return sp_finish(ctx, rc, "mixture top-n");  // (the uploads read the caller's buffer and `comps`)
}
