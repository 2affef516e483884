// ppca_robust.hip -- the streaming sweep behind Student-t PPCA (TPPCAModel).
//
// For a row with observed set O (m = |O|), model (sigma, C, mean), degrees of freedom nu, and the row's posterior mean z and Gaussian
// log-density llk_g (the posterior pass of ppca_infer / ppca_llk wrote both into scratch):
//     x~_j = x_j - mean_j,  r_j = x~_j - c_j . z  (j in O)
//     delta = (|r|^2 + sigma^2 |z|^2) / sigma^2        (= x~^T (C_O C_O^T + sigma^2 I)^-1 x~: non-negative terms, no cancellation)
//     u     = (nu + m) / (nu + delta)
//     ell   = lg[m] - 1/2 logdet - 1/2 (nu + m) log1p(delta / nu),  logdet = -2 llk_g - m ln 2 pi - delta
//     y_j   = fl(fl(sqrt(u)) * fl(x~_j)) on observed entries, NaN on masked ones                                 (YOUT)
//     V_j = sum_i w u m_ij z_i (k) | A_j = sum w u m x~_j | T_j = sum w u m | sq_j = sum w u m x~_j^2          (SUMS)
//     scalars: sum w | sum w ell | sum w (g[m] + ln u - u) | rows with m > 0
// A row without an observed entry has delta = 0, u = 1, ell = 0.
//
// Layout: a thread owns CPL columns, tcol + c * (threads per row), for every row it sees, so its rows of C (CPL x KB doubles), its
// means and its k + 3 sums per column stay in registers for the whole run.  d <= 256: one wave per row (64 threads per row, four rows
// per workgroup step), the row reductions are 64-lane butterflies without a barrier.  d > 256: the workgroup's 256 threads share a
// row; the butterflies' results of the four waves meet in LDS in wave order.  RU row steps are in flight per thread (non-temporal
// loads, as ppca_scale.hip).  A workgroup takes one contiguous run of rows (persistent grid); the column sums of its waves are added
// in wave order in LDS and go to part[workgroup][plen], and launch_reduce_partials adds the workgroups in its fixed order: no float
// atomics, bit-reproducible for a given grid.  delta, u, ell and y depend on their row alone (the lane <-> column map is fixed by
// d), hence not on the grid, the chunk or a slice's offset.
#include <algorithm>

#include "ppca_device.hpp"

namespace ppca {
namespace {

constexpr int ROBUST_THREADS = 256;
// row steps a thread has in flight (two where the registers hold 4 x 16 entries of C and 4 x 19 sums)
__host__ __device__ constexpr int robust_ru(int kb, int cpl) { return kb == 16 && cpl == 4 ? 2 : 4; }
// the state sizes a thread's registers are laid out for: the smallest of 4, 8, 12, 16 that covers k
constexpr int robust_kb(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 12 ? 12 : 16)); }

struct RobustArgs {
    const double *X;
    int64_t ldx, n;
    int d, k;
    const double *w;       // nullable (= 1)
    const double *model;   // [sigma, sigma^2, ln sigma, 0 | C (d x k) | mean (d)]
    const double *llks;    // n: Gaussian log-densities of the rows
    const double *states;  // n x k: posterior means
    const double *tabs;    // [lg (d + 1) | g (d + 1)]
    double nu;
    double *Y;             // n x d (row stride d), YOUT only
    double *u, *maha, *ell;  // nullable, n
    double *part;          // [grid][plen], plen = (SUMS ? (k + 3) d : 0) + 4
    int64_t rows_per_wg;
};

// v of lane l (uniform) on every lane
__device__ __forceinline__ double lane_bcast(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

template <int KB, int CPL, bool WIDE, bool YOUT, bool SUMS>
__global__ __launch_bounds__(ROBUST_THREADS) void robust_kernel(RobustArgs a) {
    constexpr int RU = robust_ru(KB, CPL);
    __shared__ double red[4][64];
    __shared__ double rsum[2][RU][4];
    __shared__ double zs[4][RU * KB];  // per wave: the posterior means of its rows in flight (each wave reads only its own copy)
    __shared__ double tl[2 * (ROBUST_MAX_D + 1)];  // [lg | g]
    constexpr int CS = WIDE ? ROBUST_THREADS : 64;  // threads per row = column stride of a thread's slots
    constexpr int RPS = WIDE ? 1 : 4;               // rows per step of the workgroup
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wrow = WIDE ? 0 : wave;
    const int d = a.d, k = a.k;
    const int tcol = WIDE ? t : lane;
    const double s2 = a.model[1], nu = a.nu;
    const double *__restrict__ C = a.model + MODEL_HDR;
    const double *__restrict__ mu = C + (int64_t)d * k;
    const double qnan = __builtin_nan("");
    const int64_t plen = (SUMS ? (int64_t)(k + 3) * d : 0) + 4;

    for (int e = t; e < 2 * (d + 1); e += ROBUST_THREADS) tl[e] = a.tabs[e];
    double c[CPL][KB], mj[CPL];
    bool on[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        const int j = cc * CS + tcol;
        on[cc] = j < d;
        mj[cc] = on[cc] ? mu[j] : 0.0;
#pragma unroll
        for (int b = 0; b < KB; ++b) c[cc][b] = (on[cc] && b < k) ? C[(int64_t)j * k + b] : 0.0;
    }
    double acc[SUMS ? CPL : 1][KB + 3];
    if constexpr (SUMS) {
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc)
#pragma unroll
            for (int q = 0; q < KB + 3; ++q) acc[cc][q] = 0.0;
    }
    double sw = 0.0, swl = 0.0, swq = 0.0, sne = 0.0;  // lane u < RU: the scalars of the rows it did the arithmetic of
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_wg, r1 = r0 + a.rows_per_wg < a.n ? r0 + a.rows_per_wg : a.n;
    // What the NEXT step needs is requested before this step's arithmetic: the rows' entries, and spread over the lanes the rows'
    // posterior means (lane u KB + b: z_b of row step u, 0 beyond k or the run), Gaussian log-densities and weights (lane u).
    double xn[RU][CPL], zn = 0.0, ln = 0.0, wn = 0.0;
    auto fetch = [&](int64_t rbn) {
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int64_t r = rbn + (int64_t)u * RPS + wrow;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc)
                xn[u][cc] = (r < r1 && on[cc]) ? __builtin_nontemporal_load(a.X + r * a.ldx + (cc * CS + tcol)) : qnan;
        }
        if (lane < RU * KB) {
            const int u = lane / KB, b = lane % KB;
            const int64_t r = rbn + (int64_t)u * RPS + wrow;
            zn = (b < k && r < r1) ? a.states[r * k + b] : 0.0;
        }
        if (lane < RU) {
            const int64_t r = rbn + (int64_t)lane * RPS + wrow;
            ln = r < r1 ? a.llks[r] : 0.0;
            wn = r < r1 ? (a.w ? a.w[r] : 1.0) : 0.0;
        }
    };
    fetch(r0);
    for (int64_t rb = r0; rb < r1; rb += (int64_t)RPS * RU) {  // (uniform over the workgroup: the wide form meets at barriers)
        double x[RU][CPL], ss[RU], mc[RU];
        unsigned obs[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u)
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) x[u][cc] = xn[u][cc];
        const double lk = ln, wl = wn;
        __builtin_amdgcn_wave_barrier();  // (the reads of the step before are done: LDS serves a wave in order)
        if (lane < RU * KB) zs[wave][lane] = zn;
        __builtin_amdgcn_wave_barrier();
        fetch(rb + (int64_t)RPS * RU);
        // the residuals' squares and the counts of the rows in flight
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            double z[KB];
#pragma unroll
            for (int b = 0; b < KB; ++b) z[b] = zs[wave][u * KB + b];
            ss[u] = 0.0;
            mc[u] = 0.0;
            obs[u] = 0u;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const bool o = __builtin_isfinite(x[u][cc]);
                const double xt = o ? __dsub_rn(x[u][cc], mj[cc]) : 0.0;
                double dot = 0.0;
#pragma unroll
                for (int b = 0; b < KB; ++b) dot = fma(c[cc][b], z[b], dot);
                const double res = o ? xt - dot : 0.0;
                ss[u] = fma(res, res, ss[u]);
                mc[u] += o ? 1.0 : 0.0;
                obs[u] |= o ? (1u << cc) : 0u;
                x[u][cc] = xt;
            }
            ss[u] = wave_total(ss[u]);  // (DPP steps in a fixed order; the total on every lane)
            mc[u] = wave_total(mc[u]);
        }
        if constexpr (WIDE) {  // the four waves of the row, in wave order
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    rsum[0][u][wave] = ss[u];
                    rsum[1][u][wave] = mc[u];
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                ss[u] = ((rsum[0][u][0] + rsum[0][u][1]) + rsum[0][u][2]) + rsum[0][u][3];
                mc[u] = ((rsum[1][u][0] + rsum[1][u][1]) + rsum[1][u][2]) + rsum[1][u][3];
            }
            __syncthreads();
        }
        // the rows' own arithmetic (a division, two logarithms, a square root), lane u for row step u instead of every lane for each
        double ub, su;
        {
            double mss = 0.0, mmc = 0.0;
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                mss = lane == u ? ss[u] : mss;
                mmc = lane == u ? mc[u] : mmc;
            }
            const int lu = lane < RU ? lane : 0;
            double zz = 0.0;
#pragma unroll
            for (int b = 0; b < KB; ++b) {
                const double zb = zs[wave][lu * KB + b];
                zz = fma(zb, zb, zz);
            }
            const int m = (int)mmc;
            const double md = (double)m;
            const double delta = m > 0 ? fma(s2, zz, mss) / s2 : 0.0;
            ub = m > 0 ? (nu + md) / (nu + delta) : 1.0;
            const double logdet = -2.0 * lk - md * LN_2PI - delta;
            const double el = m > 0 ? tl[m] - 0.5 * logdet - 0.5 * (nu + md) * log1p(delta / nu) : 0.0;
            su = sqrt(ub);
            const int64_t r = rb + (int64_t)lu * RPS + wrow;
            if (lane < RU && r < r1) {
                if (!WIDE || wave == 0) {
                    if (a.u) a.u[r] = ub;
                    if (a.maha) a.maha[r] = delta;
                    if (a.ell) a.ell[r] = el;
                }
                sw += wl;
                swl = fma(wl, el, swl);
                swq = fma(wl, tl[d + 1 + m] + log(ub) - ub, swq);
                sne += m > 0 ? 1.0 : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int64_t r = rb + (int64_t)u * RPS + wrow;
            const bool live = r < r1;
            const double su_u = lane_bcast(su, u);
            const double wu = lane_bcast(wl, u) * lane_bcast(ub, u);  // (a dead row's weight is 0)
            double z[SUMS ? KB : 1];
            if constexpr (SUMS) {
#pragma unroll
                for (int b = 0; b < KB; ++b) z[b] = zs[wave][u * KB + b];
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const bool o = (obs[u] >> cc) & 1u;
                const double xt = x[u][cc];
                if constexpr (YOUT) {
                    if (live && on[cc]) __builtin_nontemporal_store(o ? __dmul_rn(su_u, xt) : qnan, a.Y + r * d + (cc * CS + tcol));
                }
                if constexpr (SUMS) {
                    const double wm = o ? wu : 0.0;
#pragma unroll
                    for (int b = 0; b < KB; ++b) acc[cc][b] = fma(wm, z[b], acc[cc][b]);
                    acc[cc][KB] = fma(wm, xt, acc[cc][KB]);
                    acc[cc][KB + 1] += wm;
                    acc[cc][KB + 2] = fma(wm * xt, xt, acc[cc][KB + 2]);
                }
            }
        }
    }

    double *part = a.part + (int64_t)blockIdx.x * plen;
    if constexpr (SUMS) {
        // V (d x k) | A | T | sq; the narrow form adds its four waves (the same columns each) in wave order
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int j = cc * CS + tcol;
#pragma unroll
            for (int q = 0; q < KB + 3; ++q) {
                const bool used = q >= KB || q < k;  // (uniform)
                if (!used) continue;
                const int64_t at = q < KB ? (int64_t)j * k + q : (int64_t)d * k + (int64_t)(q - KB) * d + j;
                if constexpr (WIDE) {
                    if (on[cc]) part[at] = acc[cc][q];
                } else {
                    red[wave][lane] = acc[cc][q];
                    __syncthreads();
                    if (wave == 0 && on[cc]) part[at] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
                    __syncthreads();
                }
            }
        }
    }
    // the scalars: the wave's row-step lanes in order, then (narrow form) the waves in order
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        tot[0] += lane_bcast(sw, u);
        tot[1] += lane_bcast(swl, u);
        tot[2] += lane_bcast(swq, u);
        tot[3] += lane_bcast(sne, u);
    }
    double *sc = part + plen - 4;
    if constexpr (WIDE) {
        if (t == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sc[q] = tot[q];
        }
    } else {
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[wave][q] = tot[q];
        }
        __syncthreads();
        if (t < 4) sc[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

template <int KB, int CPL, bool WIDE>
void launch_mode(bool yout, bool sums, dim3 g, hipStream_t s, const RobustArgs &a) {
    const dim3 b(ROBUST_THREADS);
    if (yout)
        hipLaunchKernelGGL((robust_kernel<KB, CPL, WIDE, true, true>), g, b, 0, s, a);
    else if (sums)
        hipLaunchKernelGGL((robust_kernel<KB, CPL, WIDE, false, true>), g, b, 0, s, a);
    else
        hipLaunchKernelGGL((robust_kernel<KB, CPL, WIDE, false, false>), g, b, 0, s, a);
}

template <int KB>
void launch_shape(bool yout, bool sums, dim3 g, hipStream_t s, const RobustArgs &a) {
    if (a.d <= 64)
        launch_mode<KB, 1, false>(yout, sums, g, s, a);
    else if (a.d <= 256)
        launch_mode<KB, 4, false>(yout, sums, g, s, a);
    else
        launch_mode<KB, 4, true>(yout, sums, g, s, a);
}

}  // namespace

bool robust_covers(int d, int k) { return d >= 1 && d <= ROBUST_MAX_D && k >= 1 && k <= ROBUST_MAX_K; }

int64_t robust_plen(int d, int k, bool sums) { return (sums ? (int64_t)(k + 3) * d : 0) + 4; }

// Rows a workgroup takes per step: its run of rows is a multiple of that.
static int robust_step(int d, int k) { return (d <= 256 ? 4 : 1) * robust_ru(robust_kb(k), d <= 64 ? 1 : 4); }

int robust_grid(int64_t n, int d, int k, int n_cu) {
    if (n <= 0) return 0;
    const int64_t step = robust_step(d, k);
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(n_cu, 1) * 4, (n + step - 1) / step));
}

hipError_t launch_robust_sweep(const double *X, int64_t ldx, const double *w, int64_t n, int d, int k, const double *model,
                               const double *llks, const double *states, const double *tabs, double nu, double *Y, bool sums, double *u,
                               double *maha, double *ell, double *part, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    if (!robust_covers(d, k)) return hipErrorInvalidValue;
    const int64_t step = robust_step(d, k);
    const int64_t per = ((n + grid - 1) / grid + step - 1) / step * step;
    RobustArgs a{X, ldx, n, d, k, w, model, llks, states, tabs, nu, Y, u, maha, ell, part, per};
    const dim3 g((unsigned)grid);
    const bool so = sums || Y != nullptr;  // (the scaled rows alone: the sums are taken and not read)
    switch (robust_kb(k)) {
        case 4: launch_shape<4>(Y != nullptr, so, g, s, a); break;
        case 8: launch_shape<8>(Y != nullptr, so, g, s, a); break;
        case 12: launch_shape<12>(Y != nullptr, so, g, s, a); break;
        default: launch_shape<16>(Y != nullptr, so, g, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace ppca
