// ppca_scale.hip -- the per-column streaming passes behind factor analysis (per-column noise):
//
//   scale_kernel   one sweep over an N x d dataset (row stride ldx) with per-column vectors a, b, l:
//                    out_ij    = x_ij a_j on observed entries (ONE fp64 multiply), NaN on masked ones        (nullable)
//                    tot_j     = sum_i w_i m_ij
//                    sum_j     = sum_i w_i m_ij (x_ij a_j - b_j)
//                    sq_j      = sum_i w_i m_ij (x_ij a_j - b_j)^2
//                    rowsum_i  = sum_j m_ij l_j                                                              (nullable)
//                  With a = 1 / psi, b = mean / psi it whitens the dataset for the EM pass of PPCAModel(1, A, mean~) and takes the
//                  one sum of squares the packed statistics lack; with l = ln psi it gives the rows' Jacobian terms of llks.
//   fill_kernel    out_ij = x_ij (bit-exact) where x is observed, fill_ij a_j elsewhere (FAModel.extrapolate).
//   moments_multi_kernel   scale_kernel's three column sums for K row-weight vectors e[c][i] (used INSTEAD of the dataset's weights)
//                  and K offset vectors b_c in ONE sweep (the mixture of factor analysers):
//                    tot_cj = sum_i e_ci m_ij,  sum_cj = sum_i e_ci m_ij (x_ij a_j - b_cj),  sq_cj = sum_i e_ci m_ij (x_ij a_j - b_cj)^2
//                  Every element is centred on its OWN component's b_cj before it is squared (no common pivot corrected afterwards:
//                  with the components' means many standard deviations apart that correction cancels).
//
// scale_kernel is bandwidth bound: a thread owns one 16-byte column pair (d even, rows 16-byte aligned; one column otherwise) of
// SCALE_ROWS rows per step, so that a wave's load is one contiguous 1 KiB segment and SCALE_ROWS of them are requested before the
// first is used.  The 256 threads are cut as (rows per step) x (threads per row, a power of two >= the column slots, at most 256);
// rows wider than 256 slots are walked in blocks of 256 slots, each block over the workgroup's whole run of rows, so that the
// column sums live in registers whatever d is.  A workgroup takes one contiguous run of rows (persistent grid); its column sums go
// to part[workgroup][3 d] through a fixed-order sum over the row groups in LDS, and launch_reduce_partials adds the workgroups in
// its fixed order: no float atomics, bit-reproducible for a given grid.  out and rowsum depend on their row alone (the row sum is
// a 64-lane butterfly, then the row's waves in index order, then the column blocks in order), hence not on the grid.
//
// moments_multi_kernel keeps that layout (column pair per thread, SCALE_ROWS rows in flight, non-temporal loads, persistent grid,
// column sums in registers for any d, fixed-order partials part[workgroup][K][3][d], no float atomics).  A thread holds the
// 3 x VEC sums of KB components at once (KB = 1, 2, 4 or 8: the smallest that covers K, MULTI_KB_MAX = 8 beyond); K > 8 takes the
// components in blocks of 8, each block over the workgroup's run of rows again (at K <= 8 X is read once).  The weights of a
// row are read once per row and component by every thread of the row: the same address across the row's lanes.
// The mask enters as a factor 1 / 0 on the weight, not as a select on the term: the offsets b_cj must be finite (a masked entry's
// term is 0 * (0 - b_cj)), where scale_kernel's select form would ignore a non-finite offset on masked entries.
#include <algorithm>

#include "ppca_sweep.hpp"

namespace ppca {
namespace {

constexpr int SCALE_THREADS = 256;
constexpr int SCALE_ROWS = 4;  // row steps a thread has in flight

struct ScaleArgs {
    const double *X;
    int64_t ldx, n;
    int d;
    const double *w;       // nullable (= 1)
    const double *abl;     // [3][d]: a, b, l
    double *out;           // nullable, n x d (row stride d)
    double *part;          // [grid][3 d]: tot, sum, sq
    double *rowsum;        // nullable, n
    int tpr_log2;          // threads per row = 1 << tpr_log2
    int64_t rows_per_wg;
};

template <int VEC, bool ROWSUM>
__global__ __launch_bounds__(SCALE_THREADS) void scale_kernel(ScaleArgs a) {
    __shared__ double red[SCALE_THREADS];
    __shared__ double rs[SCALE_ROWS][4];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<SCALE_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    double *part = a.part + (int64_t)blockIdx.x * 3 * d;
    const double qnan = __builtin_nan("");
    for (int c0 = 0; c0 < slots; c0 += tpr) {
        const int slot = c0 + tc;
        const bool on = slot < slots;
        const int j = slot * VEC;
        double av[VEC], bv[VEC], lv[VEC], tot[VEC], sum[VEC], sq[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            av[v] = on ? a.abl[j + v] : 0.0;
            bv[v] = on ? a.abl[d + j + v] : 0.0;
            lv[v] = on ? a.abl[2 * d + j + v] : 0.0;
            tot[v] = sum[v] = sq[v] = 0.0;
        }
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * SCALE_ROWS) {  // (uniform trip count: the row sums meet at barriers)
            Vec<VEC> x[SCALE_ROWS];
            double wv[SCALE_ROWS];
#pragma unroll
            for (int u = 0; u < SCALE_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                const bool live = on && r < r1;
                if (live) {
                    x[u] = load_vec<VEC, true>(a.X + r * a.ldx + j);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u].v[v] = qnan;
                }
                wv[u] = (live && a.w) ? a.w[r] : 1.0;
            }
            double ls[SCALE_ROWS];
#pragma unroll
            for (int u = 0; u < SCALE_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                Vec<VEC> y;
                ls[u] = 0.0;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const bool obs = __builtin_isfinite(x[u].v[v]);
                    const double yv = __dmul_rn(x[u].v[v], av[v]);  // (kept apart from the subtraction: out is the plain product)
                    const double e = obs ? __dsub_rn(yv, bv[v]) : 0.0;
                    const double wm = obs ? wv[u] : 0.0;
                    tot[v] += wm;
                    sum[v] = fma(wm, e, sum[v]);
                    sq[v] = fma(wm * e, e, sq[v]);
                    y.v[v] = obs ? yv : qnan;
                    if (ROWSUM) ls[u] += obs ? lv[v] : 0.0;
                }
                if (a.out && on && r < r1) store_vec<VEC, true>(a.out + r * d + j, y);
            }
            if constexpr (ROWSUM) {
                // the row's threads: a butterfly over min(tpr, 64) lanes (groups are aligned powers of two), then its waves in order
#pragma unroll
                for (int u = 0; u < SCALE_ROWS; ++u)
                    for (int off = (tpr < 64 ? tpr : 64) >> 1; off > 0; off >>= 1) ls[u] += __shfl_xor(ls[u], off, 64);
                if (tpr > 64) {
                    if ((t & 63) == 0)
#pragma unroll
                        for (int u = 0; u < SCALE_ROWS; ++u) rs[u][t >> 6] = ls[u];
                    __syncthreads();
                    const int wpr = tpr >> 6, w0 = tr * wpr;
#pragma unroll
                    for (int u = 0; u < SCALE_ROWS; ++u) {
                        double s = rs[u][w0];
                        for (int q = 1; q < wpr; ++q) s += rs[u][w0 + q];
                        ls[u] = s;
                    }
                    __syncthreads();
                }
                if (tc == 0)
#pragma unroll
                    for (int u = 0; u < SCALE_ROWS; ++u) {
                        const int64_t r = rb + (int64_t)u * rps + tr;
                        if (r < r1) a.rowsum[r] = c0 == 0 ? ls[u] : a.rowsum[r] + ls[u];  // (the same thread wrote it in the block before)
                    }
            }
        }
        // column sums of the block: the row groups in index order
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                red[t] = q == 0 ? tot[v] : (q == 1 ? sum[v] : sq[v]);
                __syncthreads();
                if (tr == 0 && on) {
                    double s = red[tc];
                    for (int g = 1; g < rps; ++g) s += red[g * tpr + tc];
                    part[(int64_t)q * d + j + v] = s;
                }
                __syncthreads();
            }
    }
}

// out = x where x is observed (the bits as they are), fill * a_j elsewhere.  Thread = element (pair), grid-stride.
template <int VEC>
__global__ __launch_bounds__(SCALE_THREADS) void fill_kernel(const double *X, int64_t ldx, const double *F, int64_t ldf, int64_t n, int d,
                                                            const double *a, double *out) {
    const int slots = (d + VEC - 1) / VEC;
    const int64_t total = n * slots;
    for (int64_t e = (int64_t)blockIdx.x * SCALE_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * SCALE_THREADS) {
        const int64_t r = e / slots;
        const int j = (int)(e - r * slots) * VEC;
        const Vec<VEC> x = load_vec<VEC, false>(X + r * ldx + j), f = load_vec<VEC, false>(F + r * ldf + j);
        Vec<VEC> y;
#pragma unroll
        for (int v = 0; v < VEC; ++v) y.v[v] = __builtin_isfinite(x.v[v]) ? x.v[v] : __dmul_rn(f.v[v], a[j + v]);
        store_vec<VEC, false>(out + r * d + j, y);
    }
}

// ---- the column sums of K weight vectors in one sweep
constexpr int MULTI_KB_MAX = 8;  // components whose sums a thread holds at once (3 x VEC x KB doubles)

struct MultiArgs {
    const double *X;
    int64_t ldx, n;
    int d, nc;
    const double *e;       // [nc][n] row weights, component-major
    const double *a;       // nullable (= 1), d
    const double *b;       // [nc][d]
    double *part;          // [grid][nc][3][d]: tot, sum, sq of every component
    int tpr_log2;
    int64_t rows_per_wg;
};

template <int VEC, int KB>
__global__ __launch_bounds__(SCALE_THREADS) void moments_multi_kernel(MultiArgs a) {
    __shared__ double red[SCALE_THREADS];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<SCALE_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    double *part = a.part + (int64_t)blockIdx.x * a.nc * 3 * d;
    const double qnan = __builtin_nan("");
    for (int c0 = 0; c0 < slots; c0 += tpr) {
        const int slot = c0 + tc;
        const bool on = slot < slots;
        const int j = slot * VEC;
        double av[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) av[v] = (on && a.a) ? a.a[j + v] : 1.0;
        for (int k0 = 0; k0 < a.nc; k0 += KB) {  // (one trip when nc <= KB)
            const int kn = a.nc - k0 < KB ? a.nc - k0 : KB;
            double bv[KB][VEC], tot[KB][VEC], sum[KB][VEC], sq[KB][VEC];
#pragma unroll
            for (int q = 0; q < KB; ++q)
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    bv[q][v] = (on && q < kn) ? a.b[(int64_t)(k0 + q) * d + j + v] : 0.0;
                    tot[q][v] = sum[q][v] = sq[q][v] = 0.0;
                }
            for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * SCALE_ROWS) {
                Vec<VEC> x[SCALE_ROWS];
#pragma unroll
                for (int u = 0; u < SCALE_ROWS; ++u) {
                    const int64_t r = rb + (int64_t)u * rps + tr;
                    if (on && r < r1) {
                        x[u] = load_vec<VEC, true>(a.X + r * a.ldx + j);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) x[u].v[v] = qnan;
                    }
                }
#pragma unroll
                for (int u = 0; u < SCALE_ROWS; ++u) {
                    const int64_t r = rb + (int64_t)u * rps + tr;
                    const bool live = on && r < r1;
                    const int64_t rr = r < r1 ? r : r1 - 1;  // (loads without a branch: a dead row or component re-reads a live one's weight)
                    double wv[KB];
#pragma unroll
                    for (int q = 0; q < KB; ++q) {
                        const double w = a.e[(int64_t)(k0 + (q < kn ? q : kn - 1)) * a.n + rr];
                        wv[q] = (live && q < kn && __builtin_isfinite(w)) ? w : 0.0;  // a non-finite weight counts as 0
                    }
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        // the mask as a factor 1 / 0 on the (finite) weight, one multiply per component where two 64-bit selects
                        // would stand: a masked entry's e = -b_cj is finite and meets the weight 0, so it adds exactly nothing
                        const bool obs = __builtin_isfinite(x[u].v[v]);
                        const double mk = obs ? 1.0 : 0.0;
                        const double yv = obs ? __dmul_rn(x[u].v[v], av[v]) : 0.0;
#pragma unroll
                        for (int q = 0; q < KB; ++q) {
                            const double e = __dsub_rn(yv, bv[q][v]);  // centred on the component's own offset
                            const double wm = __dmul_rn(wv[q], mk);
                            tot[q][v] += wm;
                            sum[q][v] = fma(wm, e, sum[q][v]);
                            sq[q][v] = fma(wm * e, e, sq[q][v]);
                        }
                    }
                }
            }
            // column sums of the block: per component and sum, the row groups in index order
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                if (q >= kn) break;  // (uniform over the workgroup)
#pragma unroll
                for (int m = 0; m < 3; ++m)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        red[t] = m == 0 ? tot[q][v] : (m == 1 ? sum[q][v] : sq[q][v]);
                        __syncthreads();
                        if (tr == 0 && on) {
                            double s = red[tc];
                            for (int g = 1; g < rps; ++g) s += red[g * tpr + tc];
                            part[((int64_t)(k0 + q) * 3 + m) * d + j + v] = s;
                        }
                        __syncthreads();
                    }
            }
        }
    }
}

template <int VEC>
void launch_multi_vec(int kb, dim3 g, dim3 b, hipStream_t s, const MultiArgs &a) {
    if (kb == 1)
        hipLaunchKernelGGL((moments_multi_kernel<VEC, 1>), g, b, 0, s, a);
    else if (kb == 2)
        hipLaunchKernelGGL((moments_multi_kernel<VEC, 2>), g, b, 0, s, a);
    else if (kb == 4)
        hipLaunchKernelGGL((moments_multi_kernel<VEC, 4>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((moments_multi_kernel<VEC, MULTI_KB_MAX>), g, b, 0, s, a);
}

int multi_kb(int nc) { return nc <= 1 ? 1 : (nc <= 2 ? 2 : (nc <= 4 ? 4 : MULTI_KB_MAX)); }

}  // namespace

int scale_grid(int64_t n, int d, int n_cu) {
    if (n <= 0) return 0;
    const int64_t want = (int64_t)std::max(n_cu, 1) * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, (n + 7) / 8));
}

hipError_t launch_scale_columns(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *abl_dev, double *out,
                                double *part, int grid, double *rowsum, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    const SweepCut cut = sweep_cut(d, ldx % 2 == 0, {X, out});
    ScaleArgs a{X, ldx, n, d, w, abl_dev, out, part, rowsum, cut.tpr_log2, (n + grid - 1) / grid};
    const dim3 g((unsigned)grid), b(SCALE_THREADS);
    if (cut.vec) {
        if (rowsum)
            hipLaunchKernelGGL((scale_kernel<2, true>), g, b, 0, s, a);
        else
            hipLaunchKernelGGL((scale_kernel<2, false>), g, b, 0, s, a);
    } else {
        if (rowsum)
            hipLaunchKernelGGL((scale_kernel<1, true>), g, b, 0, s, a);
        else
            hipLaunchKernelGGL((scale_kernel<1, false>), g, b, 0, s, a);
    }
    return hipGetLastError();
}

// Workgroups of the multi-component sweep: what is resident at once at the kernel's register count (KB = 8: 219 VGPRs, two waves
// per SIMD = two workgroups per CU; KB = 4: 156, three; KB <= 2: at most 113, four) -- one wave of workgroups, each with one equal
// run of rows -- which also keeps the partials, grid x K x 3 d doubles, small.
int moments_multi_grid(int64_t n, int nc, int n_cu) {
    if (n <= 0) return 0;
    const int kb = multi_kb(nc);
    const int per_cu = kb <= 2 ? 4 : (kb == 4 ? 3 : 2);
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(n_cu, 1) * per_cu, (n + 7) / 8));
}

hipError_t launch_column_moments_multi(const double *X, int64_t ldx, int64_t n, int d, const double *e_dev, int nc, const double *a_dev,
                                       const double *b_dev, double *part, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0 || nc <= 0) return hipSuccess;
    const SweepCut cut = sweep_cut(d, ldx % 2 == 0, {X});
    MultiArgs a{X, ldx, n, d, nc, e_dev, a_dev, b_dev, part, cut.tpr_log2, (n + grid - 1) / grid};
    const dim3 g((unsigned)grid), b(SCALE_THREADS);
    if (cut.vec)
        launch_multi_vec<2>(multi_kb(nc), g, b, s, a);
    else
        launch_multi_vec<1>(multi_kb(nc), g, b, s, a);
    return hipGetLastError();
}

hipError_t launch_fill_masked(const double *X, int64_t ldx, const double *F, int64_t ldf, int64_t n, int d, const double *a_dev,
                              double *out, int n_cu, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const bool vec = sweep_cut(d, ldx % 2 == 0 && ldf % 2 == 0, {X, F, out}).vec;
    const int64_t total = n * (vec ? d / 2 : d);
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(n_cu, 1) * 8, (total + SCALE_THREADS - 1) / SCALE_THREADS));
    if (vec)
        hipLaunchKernelGGL(fill_kernel<2>, dim3((unsigned)grid), dim3(SCALE_THREADS), 0, s, X, ldx, F, ldf, n, d, a_dev, out);
    else
        hipLaunchKernelGGL(fill_kernel<1>, dim3((unsigned)grid), dim3(SCALE_THREADS), 0, s, X, ldx, F, ldf, n, d, a_dev, out);
    return hipGetLastError();
}

}  // namespace ppca
