// ppca_kmeans.hip -- masked k-means on the device: the streaming passes behind ppca_dataset_kmeans_step and
// ppca_dataset_kmeans_seed.
//
//   kmeans_kernel        one sweep over an N x d dataset (row stride ldx) with nc <= 8 complete centres mu_c and a per-column scale a:
//                          dist_ic  = sum_j m_ij (a_j (x_ij - mu_cj))^2          (difference, then scale, then square; masked entries
//                                                                                 are selected out, never multiplied)
//                          label_i  = the smallest c that attains min_c dist_ic  (k0 + c; a running minimum carried in labels / dist
//                                                                                 when the centres come in blocks of 8)
//                          inertia  = sum_i w_i min_c dist_ic
//                        and, in its fused form (ACC: every centre in this launch, the row's columns in the workgroup at once),
//                          tot_cj   = sum_{i: label_i = c} w_i m_ij
//                          sum_cj   = sum_{i: label_i = c} w_i m_ij (x_ij - mu_cj)      (unscaled, centred on the OLD centre)
//                        from the x values the thread still holds when the row's label is known: one read of X per Lloyd iteration.
//   kmeans_wide_kernel   the assignment alone for rows wider than the workgroup (column blocks walked inside the row step).
//   kmeans_update_kernel the two column sums by label for 8 centres at a time from the labels of an earlier sweep (d > 512 or K > 8).
//   wd_block_kernel      sum_i w_i D_i over blocks of WD_BLOCK rows: the first level of the seeding's two-level pick.
//
// The layout is ppca_scale.hip's: a thread owns one 16-byte column pair (d even, rows 16-byte aligned; one column otherwise, two when
// such a row has more than 256 columns), KM_ROWS rows in flight, non-temporal loads, a persistent grid with one contiguous run of
// rows per workgroup, per-workgroup partials part[workgroup][K][2][d] + one inertia partial, added in the fixed order of
// launch_reduce_partials: no float atomics anywhere, bit-reproducible for a given grid.  labels and dist depend on their row alone (the
// row's distances: a butterfly over min(threads per row, 64) lanes, then the row's waves in index order), hence not on the grid.
//
// The sums of "the row's label" are register sums for all centres of the launch with the label as a predicate on the weight (the way
// moments_multi_kernel uses e_ci): 3 fp64 operations per element and centre, no LDS.
#include <algorithm>

#include "ppca_sweep.hpp"

namespace ppca {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_ROWS = 4;  // row steps a thread has in flight
constexpr int WD_BLOCK = 4096;

struct KMeansArgs {
    const double *X;
    int64_t ldx, n;
    int d;
    const double *w;    // nullable (= 1)
    const double *mu;   // [nc][d]: the centres of this launch
    const double *a;    // nullable (= 1), d
    int nc, k0, carry;  // centres in this launch; the label of mu[0]; start from labels / dist (the minimum over the blocks before)
    int32_t *labels;    // nullable (not with carry), n
    double *dist;       // nullable (not with carry), n
    double *part;       // nullable: [grid][plen]; sums at [c][2][d] (ACC, update), the inertia partial at plen - 1 (inertia != 0)
    int64_t plen;
    int inertia;
    int tpr_log2;       // threads per row = 1 << tpr_log2
    int64_t rows_per_wg;
};

// dv[NR][KB] over the row's threads: a butterfly over min(tpr, 64) lanes (groups are aligned powers of two), then the row's
// waves in index order through rs.  (uniform over the workgroup: two barriers when tpr > 64)
template <int NR, int KB>
__device__ __forceinline__ void row_reduce(double (&dv)[NR][KB], double (*rs)[4], int tpr, int tr, int t) {
#pragma unroll
    for (int u = 0; u < NR; ++u)
#pragma unroll
        for (int q = 0; q < KB; ++q)
            for (int off = (tpr < 64 ? tpr : 64) >> 1; off > 0; off >>= 1) dv[u][q] += __shfl_xor(dv[u][q], off, 64);
    if (tpr > 64) {
        if ((t & 63) == 0)
#pragma unroll
            for (int u = 0; u < NR; ++u)
#pragma unroll
                for (int q = 0; q < KB; ++q) rs[u * KB + q][t >> 6] = dv[u][q];
        __syncthreads();
        const int wpr = tpr >> 6, w0 = tr * wpr;
#pragma unroll
        for (int u = 0; u < NR; ++u)
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                double s = rs[u * KB + q][w0];
                for (int g = 1; g < wpr; ++g) s += rs[u * KB + q][w0 + g];
                dv[u][q] = s;
            }
        __syncthreads();
    }
}

// The row's label and distance from its nc reduced distances: the smallest index that attains the minimum (strict <, in index order;
// the minimum carried from the blocks before wins a tie, it belongs to a lower index).
template <int KB>
__device__ __forceinline__ void row_argmin(const double (&dv)[KB], int nc, int k0, bool carry, double dist0, int lab0, double &best,
                                           int &lab) {
    best = carry ? dist0 : dv[0];
    lab = carry ? lab0 : k0;
#pragma unroll
    for (int q = 0; q < KB; ++q)
        if ((carry || q > 0) && q < nc && dv[q] < best) {
            best = dv[q];
            lab = k0 + q;
        }
}

// The workgroup's inertia partial: the row leaders' sums, the row groups in index order.
__device__ __forceinline__ void store_inertia(const KMeansArgs &a, double *red, double inert, int tpr, int rps, int t) {
    if (!a.part || !a.inertia) return;  // (uniform)
    red[t] = inert;
    __syncthreads();
    if (t == 0) {
        double s = red[0];
        for (int g = 1; g < rps; ++g) s += red[g * tpr];
        a.part[(int64_t)blockIdx.x * a.plen + a.plen - 1] = s;
    }
    __syncthreads();
}

// NS slots of VEC columns per thread: slot s * tpr + tc.  The whole row is in the workgroup at once (slots <= NS * tpr).
template <int VEC, int NS, int KB, bool ACC>
__global__ __launch_bounds__(KM_THREADS) void kmeans_kernel(KMeansArgs a) {
    constexpr int RH = (ACC && KB > 4) ? 2 : KM_ROWS;
    __shared__ double red[KM_THREADS];
    __shared__ double rs[RH * KB][4];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<KM_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    const double qnan = __builtin_nan("");
    bool on[NS];
    int j[NS];
    double av[NS][VEC], mu[KB][NS][VEC], tot[KB][NS][VEC], sum[KB][NS][VEC];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int slot = s * tpr + tc;
        on[s] = slot < slots;
        j[s] = slot * VEC;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            av[s][v] = (on[s] && a.a) ? a.a[j[s] + v] : 1.0;
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                mu[q][s][v] = (on[s] && q < a.nc) ? a.mu[(int64_t)q * d + j[s] + v] : 0.0;
                tot[q][s][v] = sum[q][s][v] = 0.0;
            }
        }
    }
    double inert = 0.0;
    for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * KM_ROWS) {  // (uniform trip count: the row sums meet at barriers)
        Vec<VEC> x[KM_ROWS][NS];
#pragma unroll
        for (int u = 0; u < KM_ROWS; ++u) {
            const int64_t r = rb + (int64_t)u * rps + tr;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (on[s] && r < r1) {
                    x[u][s] = load_vec<VEC, true>(a.X + r * a.ldx + j[s]);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u][s].v[v] = qnan;
                }
            }
        }
#pragma unroll
        for (int h = 0; h < KM_ROWS; h += RH) {  // (RH rows' distances live at once: the registers of the 8-centre form)
        double dv[RH][KB];
#pragma unroll
        for (int uh = 0; uh < RH; ++uh)
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                const int u = h + uh;
                double acc = 0.0;
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const bool obs = __builtin_isfinite(x[u][s].v[v]);
                        const double e = obs ? __dmul_rn(__dsub_rn(x[u][s].v[v], mu[q][s][v]), av[s][v]) : 0.0;
                        acc = fma(e, e, acc);
                    }
                dv[uh][q] = acc;
            }
        row_reduce<RH, KB>(dv, rs, tpr, tr, t);
#pragma unroll
        for (int uh = 0; uh < RH; ++uh) {
            const int u = h + uh;
            const int64_t r = rb + (int64_t)u * rps + tr;
            const bool live = r < r1;
            if (!ACC && !(tc == 0 && live)) continue;  // (the assignment alone: the row's leader does the rest)
            const bool carry = a.carry != 0;
            double best;
            int lab;
            row_argmin<KB>(dv[uh], a.nc, a.k0, carry, carry ? a.dist[r] : 0.0, carry ? a.labels[r] : 0, best, lab);
            const double wr = live ? (a.w ? a.w[r] : 1.0) : 0.0;
            if (tc == 0 && live) {
                if (a.labels) a.labels[r] = lab;
                if (a.dist) a.dist[r] = best;
                inert = fma(wr, best, inert);
            }
            if constexpr (ACC) {
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const bool obs = __builtin_isfinite(x[u][s].v[v]);
                        const double xv = obs ? x[u][s].v[v] : 0.0;
#pragma unroll
                        for (int q = 0; q < KB; ++q) {
                            const bool mine = obs && lab == a.k0 + q;
                            const double wm = mine ? wr : 0.0;
                            const double e = mine ? __dsub_rn(xv, mu[q][s][v]) : 0.0;
                            tot[q][s][v] += wm;
                            sum[q][s][v] = fma(wm, e, sum[q][s][v]);
                        }
                    }
            }
        }
        }
    }
    store_inertia(a, red, inert, tpr, rps, t);
    if constexpr (ACC) {
        // column sums: per centre and sum, the row groups in index order
        double *part = a.part + (int64_t)blockIdx.x * a.plen;
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            if (q >= a.nc) break;  // (uniform over the workgroup)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        red[t] = m == 0 ? tot[q][s][v] : sum[q][s][v];
                        __syncthreads();
                        if (tr == 0 && on[s]) {
                            double acc = red[tc];
                            for (int g = 1; g < rps; ++g) acc += red[g * tpr + tc];
                            part[((int64_t)(a.k0 + q) * 2 + m) * d + j[s] + v] = acc;
                        }
                        __syncthreads();
                    }
        }
    }
}

// The assignment for rows wider than the workgroup: the column blocks are walked inside the row step (a thread's partial distances run
// over its columns of every block before the row's threads meet), the centres come from memory (cache hits after the first row step).
template <int VEC, int KB>
__global__ __launch_bounds__(KM_THREADS) void kmeans_wide_kernel(KMeansArgs a) {
    __shared__ double red[KM_THREADS];
    __shared__ double rs[KM_ROWS * KB][4];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<KM_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    const double qnan = __builtin_nan("");
    double inert = 0.0;
    for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * KM_ROWS) {
        double dv[KM_ROWS][KB];
#pragma unroll
        for (int u = 0; u < KM_ROWS; ++u)
#pragma unroll
            for (int q = 0; q < KB; ++q) dv[u][q] = 0.0;
        for (int c0 = 0; c0 < slots; c0 += tpr) {
            const int slot = c0 + tc;
            const bool on = slot < slots;
            const int j = slot * VEC;
            Vec<VEC> x[KM_ROWS];
            double av[VEC], mu[KB][VEC];
#pragma unroll
            for (int u = 0; u < KM_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                if (on && r < r1) {
                    x[u] = load_vec<VEC, true>(a.X + r * a.ldx + j);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u].v[v] = qnan;
                }
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                av[v] = (on && a.a) ? a.a[j + v] : 1.0;
#pragma unroll
                for (int q = 0; q < KB; ++q) mu[q][v] = (on && q < a.nc) ? a.mu[(int64_t)q * d + j + v] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < KM_ROWS; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const bool obs = __builtin_isfinite(x[u].v[v]);
#pragma unroll
                    for (int q = 0; q < KB; ++q) {
                        const double e = obs ? __dmul_rn(__dsub_rn(x[u].v[v], mu[q][v]), av[v]) : 0.0;
                        dv[u][q] = fma(e, e, dv[u][q]);
                    }
                }
        }
        row_reduce<KM_ROWS, KB>(dv, rs, tpr, tr, t);
#pragma unroll
        for (int u = 0; u < KM_ROWS; ++u) {
            const int64_t r = rb + (int64_t)u * rps + tr;
            if (!(tc == 0 && r < r1)) continue;
            const bool carry = a.carry != 0;
            double best;
            int lab;
            row_argmin<KB>(dv[u], a.nc, a.k0, carry, carry ? a.dist[r] : 0.0, carry ? a.labels[r] : 0, best, lab);
            if (a.labels) a.labels[r] = lab;
            if (a.dist) a.dist[r] = best;
            inert = fma(a.w ? a.w[r] : 1.0, best, inert);
        }
    }
    store_inertia(a, red, inert, tpr, rps, t);
}

// tot / sum by label for the nc <= KB centres k0 .. k0 + nc of this launch (scale_kernel's walk: the column blocks outside, each over
// the workgroup's whole run of rows, so that the column sums live in registers whatever d is).
template <int VEC, int KB>
__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(KMeansArgs a) {
    __shared__ double red[KM_THREADS];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<KM_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    double *part = a.part + (int64_t)blockIdx.x * a.plen;
    const double qnan = __builtin_nan("");
    for (int c0 = 0; c0 < slots; c0 += tpr) {
        const int slot = c0 + tc;
        const bool on = slot < slots;
        const int j = slot * VEC;
        double mu[KB][VEC], tot[KB][VEC], sum[KB][VEC];
#pragma unroll
        for (int q = 0; q < KB; ++q)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                mu[q][v] = (on && q < a.nc) ? a.mu[(int64_t)q * d + j + v] : 0.0;
                tot[q][v] = sum[q][v] = 0.0;
            }
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * KM_ROWS) {
            Vec<VEC> x[KM_ROWS];
            double wr[KM_ROWS];
            int lab[KM_ROWS];
#pragma unroll
            for (int u = 0; u < KM_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                const bool live = on && r < r1;
                if (live) {
                    x[u] = load_vec<VEC, true>(a.X + r * a.ldx + j);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u].v[v] = qnan;
                }
                wr[u] = live ? (a.w ? a.w[r] : 1.0) : 0.0;
                lab[u] = live ? a.labels[r] : -1;
            }
#pragma unroll
            for (int u = 0; u < KM_ROWS; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const bool obs = __builtin_isfinite(x[u].v[v]);
                    const double xv = obs ? x[u].v[v] : 0.0;
#pragma unroll
                    for (int q = 0; q < KB; ++q) {
                        const bool mine = obs && lab[u] == a.k0 + q;
                        const double wm = mine ? wr[u] : 0.0;
                        const double e = mine ? __dsub_rn(xv, mu[q][v]) : 0.0;
                        tot[q][v] += wm;
                        sum[q][v] = fma(wm, e, sum[q][v]);
                    }
                }
        }
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            if (q >= a.nc) break;  // (uniform over the workgroup)
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    red[t] = m == 0 ? tot[q][v] : sum[q][v];
                    __syncthreads();
                    if (tr == 0 && on) {
                        double acc = red[tc];
                        for (int g = 1; g < rps; ++g) acc += red[g * tpr + tc];
                        part[((int64_t)(a.k0 + q) * 2 + m) * d + j + v] = acc;
                    }
                    __syncthreads();
                }
        }
    }
}

// out[b] = sum over rows [b WD_BLOCK, (b + 1) WD_BLOCK) of w_i D_i (w, D nullable = 1): a thread's rows in order, then a fixed tree.
__global__ __launch_bounds__(KM_THREADS) void wd_block_kernel(const double *w, const double *D, int64_t n, double *out) {
    __shared__ double red[KM_THREADS];
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * WD_BLOCK, b1 = b0 + WD_BLOCK < n ? b0 + WD_BLOCK : n;
    double s = 0.0;
    for (int64_t r = b0 + t; r < b1; r += KM_THREADS) s += (w ? w[r] : 1.0) * (D ? D[r] : 1.0);
    red[t] = s;
    __syncthreads();
    for (int off = KM_THREADS >> 1; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = red[0];
}

int kmeans_kb(int nc) { return nc <= 1 ? 1 : (nc <= 4 ? 4 : KMEANS_KB_MAX); }

template <int VEC, int NS, bool ACC>
void launch_row(int kb, dim3 g, dim3 b, hipStream_t s, const KMeansArgs &a) {
    if (kb == 1)
        hipLaunchKernelGGL((kmeans_kernel<VEC, NS, 1, ACC>), g, b, 0, s, a);
    else if (kb == 4)
        hipLaunchKernelGGL((kmeans_kernel<VEC, NS, 4, ACC>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((kmeans_kernel<VEC, NS, KMEANS_KB_MAX, ACC>), g, b, 0, s, a);
}

template <int VEC>
void launch_wide(int kb, dim3 g, dim3 b, hipStream_t s, const KMeansArgs &a) {
    if (kb == 1)
        hipLaunchKernelGGL((kmeans_wide_kernel<VEC, 1>), g, b, 0, s, a);
    else if (kb == 4)
        hipLaunchKernelGGL((kmeans_wide_kernel<VEC, 4>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((kmeans_wide_kernel<VEC, KMEANS_KB_MAX>), g, b, 0, s, a);
}

template <int VEC>
void launch_update(int kb, dim3 g, dim3 b, hipStream_t s, const KMeansArgs &a) {
    if (kb == 1)
        hipLaunchKernelGGL((kmeans_update_kernel<VEC, 1>), g, b, 0, s, a);
    else if (kb == 4)
        hipLaunchKernelGGL((kmeans_update_kernel<VEC, 4>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((kmeans_update_kernel<VEC, KMEANS_KB_MAX>), g, b, 0, s, a);
}

}  // namespace

// One wave of workgroups, each with one equal run of rows: what is resident at once at the fused kernel's register count.
int kmeans_grid(int64_t n, int nc, int n_cu) {
    if (n <= 0) return 0;
    const int kb = kmeans_kb(std::min(nc, KMEANS_KB_MAX));
    const int per_cu = kb <= 1 ? 4 : (kb == 4 ? 3 : 2);
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(n_cu, 1) * per_cu, (n + 7) / 8));
}

hipError_t launch_kmeans_assign(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *mu_dev, const double *a_dev,
                                int nc, int k0, int carry, int32_t *labels, double *dist, bool accumulate, double *part, int64_t plen,
                                int inertia, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    if (nc < 1 || nc > KMEANS_KB_MAX || (carry && (!labels || !dist)) || ((accumulate || inertia) && !part)) return hipErrorInvalidValue;
    const auto [vec, slots, lg] = sweep_cut(d, ldx % 2 == 0, {X});
    const int ns = slots <= KM_THREADS ? 1 : ((!vec && slots <= 2 * KM_THREADS) ? 2 : 0);  // 0: wider than the workgroup
    if (accumulate && (ns == 0 || carry || k0 != 0)) return hipErrorInvalidValue;
    KMeansArgs a{X, ldx, n, d, w, mu_dev, a_dev, nc, k0, carry, labels, dist, part, plen, inertia,
                 ns == 2 ? sweep_tpr_log2((slots + 1) / 2) : lg, (n + grid - 1) / grid};
    const dim3 g((unsigned)grid), b(KM_THREADS);
    const int kb = kmeans_kb(nc);
    if (ns == 0) {
        if (vec)
            launch_wide<2>(kb, g, b, s, a);
        else
            launch_wide<1>(kb, g, b, s, a);
    } else if (accumulate) {
        if (vec)
            launch_row<2, 1, true>(kb, g, b, s, a);
        else if (ns == 1)
            launch_row<1, 1, true>(kb, g, b, s, a);
        else
            launch_row<1, 2, true>(kb, g, b, s, a);
    } else {
        if (vec)
            launch_row<2, 1, false>(kb, g, b, s, a);
        else if (ns == 1)
            launch_row<1, 1, false>(kb, g, b, s, a);
        else
            launch_row<1, 2, false>(kb, g, b, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_kmeans_update(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *mu_dev, int nc, int k0,
                                const int32_t *labels, double *part, int64_t plen, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    if (nc < 1 || nc > KMEANS_KB_MAX || !labels || !part) return hipErrorInvalidValue;
    const SweepCut cut = sweep_cut(d, ldx % 2 == 0, {X});
    KMeansArgs a{X, ldx, n, d, w, mu_dev, nullptr, nc, k0, 0, const_cast<int32_t *>(labels), nullptr, part, plen, 0, cut.tpr_log2,
                 (n + grid - 1) / grid};
    const dim3 g((unsigned)grid), b(KM_THREADS);
    if (cut.vec)
        launch_update<2>(kmeans_kb(nc), g, b, s, a);
    else
        launch_update<1>(kmeans_kb(nc), g, b, s, a);
    return hipGetLastError();
}

int64_t wd_blocks(int64_t n) { return (n + WD_BLOCK - 1) / WD_BLOCK; }
int64_t wd_block_rows() { return WD_BLOCK; }

hipError_t launch_wd_block_sums(const double *w, const double *dist, int64_t n, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(wd_block_kernel, dim3((unsigned)wd_blocks(n)), dim3(KM_THREADS), 0, s, w, dist, n, out);
    return hipGetLastError();
}

}  // namespace ppca
