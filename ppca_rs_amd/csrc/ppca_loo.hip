// ppca_loo.hip -- the leave-one-out predictive of every entry (ppca_loo_predictive, ppca_mix_loo_predictive).
//
// For a row with observed set O, posterior mean z and covariance Sigma = sigma^2 M^-1 (what ppca_infer returns), model
// (sigma, C, mean) and c_j the j-th row of C:
//     r_j = x_j - mean_j - c_j^T z,   q_j = c_j^T Sigma c_j,   s_j = sigma^2 - q_j = sigma^2 (1 - h_j)
//     observed j: mean x_j - sigma^2 r_j / s_j, variance sigma^4 / s_j, l_j = -1/2 (log 2 pi + log(sigma^4 / s_j) + r_j^2 / s_j)
//     masked j:   mean mean_j + c_j^T z (= extrapolate), variance sigma^2 + q_j (the extrapolated covariance diagonal)
// which is the predictive of x_j given the row's other observed entries, the model held fixed.  Exactly, sigma^4 / s_j =
// sigma^2 + c_j^T Sigma_-j c_j <= sigma^2 + |c_j|^2 (the posterior covariance without j is below the prior's I), so
// s_j >= sigma^4 / (sigma^2 + |c_j|^2) > 0.  Rounding can break that when h_j -> 1 (the entry alone pins a latent direction); an
// observed entry whose s_j falls to that bound or below (s_j <= 0 included) takes the prior predictive (mean_j, sigma^2 + |c_j|^2),
// which is the exact answer at the bound (c_j orthogonal to the other observed rows of C).  DESIGN.md section 4.10.
//
// The mixture folds one component's (m, v, l) at a time into per-entry state (mix_loo_fold_kernel): for an observed entry a
// running maximum and scaled sum of t_c = lp_c - l_cj (lp_c the row's log posterior of c) and the scaled sum of t-weighted
// means; for a masked entry the sums of exp(lp_c) and exp(lp_c) m_cj, as ppca_mix_reconstruct weighs them.  mix_loo_finish_kernel
// turns that into the mean and L_j = log sum_c exp(t_c) (l_j = -L_j); a second sweep over the components adds the variance around
// the mean (mix_loo_var_kernel).
#include <algorithm>

#include "ppca_sweep.hpp"

namespace ppca {
namespace {

constexpr int LOO_THREADS = 256;

struct LooArgs {
    const double *X;       // the chunk's rows (masks and values)
    int64_t ldx;
    int d, k;
    int64_t n_rows;
    const double *model;   // [sigma, sigma^2, ln sigma, 0 | C (d x k) | mean (d)]
    const double *states;  // n_rows x k
    const double *covs;    // n_rows x k x k
    double *mean, *var;    // nullable, n_rows x d
    double *ell;           // nullable, n_rows x d: l_j of observed entries, 0 on masked ones (the mixture's fold)
    double *llks;          // nullable, n_rows: sum of l_j over the observed entries
};

// Sum over the 256 threads of a block, the same order on every run: lane butterflies down to lane 0, then the four waves in index
// order.  red: 4 doubles of LDS.  The result is returned on every thread.
__device__ __forceinline__ double block_sum256(double v, double *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int t = threadIdx.x;
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// One workgroup per row (grid-stride over the chunk), one thread per entry.  LDS: Sigma, padded to kq = pad16(k) columns with zeros,
// z padded likewise, 4 doubles of reduction.
__global__ __launch_bounds__(LOO_THREADS) void loo_kernel(LooArgs a) {
    extern __shared__ double lds[];
    const int k = a.k, d = a.d, kq = pad16(k), t = threadIdx.x;
    double *S = lds, *Z = lds + (size_t)k * kq, *red = Z + kq;
    const double sig2 = a.model[1];
    const double *C = a.model + 4;
    const double *mu = C + (int64_t)d * k;
    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const double *Sg = a.covs + r * k * k;
        for (int e = t; e < k * kq; e += LOO_THREADS) {
            const int ra = e / kq, cb = e % kq;
            S[e] = (ra < k && cb < k) ? Sg[ra * k + cb] : 0.0;
        }
        for (int e = t; e < kq; e += LOO_THREADS) Z[e] = e < k ? a.states[r * k + e] : 0.0;
        __syncthreads();
        const double *x = a.X + r * a.ldx;
        double lsum = 0.0;
        for (int j = t; j < d; j += LOO_THREADS) {
            const double *cj = C + (int64_t)j * k;
            // q = c_j^T Sigma c_j by blocks of 16 columns of Sigma (acc = c_j^T Sigma[:, b0:b0+16]); the padding columns are 0.
            // (heldout_score_kernel has this loop without cn; shared, it changed both kernels' code: change the two together)
            double dot = 0.0, cn = 0.0, q = 0.0;
            for (int b0 = 0; b0 < k; b0 += 16) {
                double acc[16];
#pragma unroll
                for (int b = 0; b < 16; ++b) acc[b] = 0.0;
                for (int i = 0; i < k; ++i) {
                    const double ci = cj[i];
                    if (b0 == 0) {
                        dot = fma(ci, Z[i], dot);
                        cn = fma(ci, ci, cn);
                    }
                    const double *Si = S + (size_t)i * kq + b0;
#pragma unroll
                    for (int b = 0; b < 16; ++b) acc[b] = fma(ci, Si[b], acc[b]);
                }
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (b0 + b < k) q = fma(acc[b], cj[b0 + b], q);
            }
            const double xv = x[j];
            const double pm = mu[j] + dot;
            double m, v, l = 0.0;
            if (!__builtin_isfinite(xv)) {
                m = pm;
                v = sig2 + q;
            } else {
                const double s = sig2 - q, vp = sig2 + cn;
                if (!(s * vp > sig2 * sig2)) {  // at or past the exact bound (or NaN): the prior predictive
                    const double r0 = xv - mu[j];
                    m = mu[j];
                    v = vp;
                    l = -0.5 * (LOG_2PI + log(vp) + r0 * r0 / vp);
                } else {
                    const double res = xv - pm;
                    m = xv - sig2 * res / s;
                    v = sig2 * sig2 / s;
                    l = -0.5 * (LOG_2PI + log(v) + res * res / s);
                }
                lsum += l;
            }
            const int64_t o = r * d + j;
            if (a.mean) a.mean[o] = m;
            if (a.var) a.var[o] = v;
            if (a.ell) a.ell[o] = l;
        }
        const double tot = block_sum256(lsum, red);  // (its barriers also keep S, Z until every thread is done with the row)
        if (a.llks && t == 0) a.llks[r] = tot;
    }
}

// Fold component c into the per-entry state of the chunk (mx, sm, wm: n_rows x d; wm nullable when no mean is wanted).
__global__ void mix_loo_fold_kernel(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                                    const double *m, const double *ell, double *mx, double *sm, double *wm, int first) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows * d) return;
    const int64_t r = e / d;
    const int j = (int)(e - r * d);
    const double lp = logpost[r * nm + c];
    double M = first ? -INFINITY : mx[e], S = first ? 0.0 : sm[e], W = first ? 0.0 : (wm ? wm[e] : 0.0);
    const double mv = wm ? m[e] : 0.0;
    if (__builtin_isfinite(X[r * ldx + j])) {
        const double tc = lp - ell[e];
        if (tc > M) {
            const double sc = exp(M - tc);
            S = S * sc + 1.0;
            W = W * sc + mv;
            M = tc;
        } else if (tc > -INFINITY) {
            const double ex = exp(tc - M);
            S += ex;
            W = fma(ex, mv, W);
        }
    } else {  // weights exp(lp_c) as they are (ppca_mix_reconstruct): the maximum stays 0
        const double ex = exp(lp);
        M = 0.0;
        S += ex;
        W = fma(ex, mv, W);
    }
    mx[e] = M;
    sm[e] = S;
    if (wm) wm[e] = W;
}

// Per row (one workgroup, grid-stride): L_j = mx + log sm of observed entries (into mx), the mean (wm / sm observed, wm masked) into
// mean (nullable; may alias wm), llks[r] = -sum_{j in O} L_j (nullable; fixed order as loo_kernel).
__global__ __launch_bounds__(LOO_THREADS) void mix_loo_finish_kernel(const double *X, int64_t ldx, int d, int64_t n_rows, double *mx,
                                                                  const double *sm, const double *wm, double *mean, double *llks) {
    __shared__ double red[4];
    for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        double lsum = 0.0;
        for (int j = threadIdx.x; j < d; j += LOO_THREADS) {
            const int64_t e = r * d + j;
            const bool obs = __builtin_isfinite(X[r * ldx + j]);
            if (obs) {
                const double L = mx[e] + log(sm[e]);
                mx[e] = L;
                lsum -= L;
            }
            if (mean) mean[e] = obs ? wm[e] / sm[e] : wm[e];
        }
        const double tot = block_sum256(lsum, red);
        if (llks && threadIdx.x == 0) llks[r] = tot;
    }
}

// var (+)= a_cj (v_cj + (m_cj - mean_j)^2), a_cj = exp(lp_c - l_cj - L_j) observed, exp(lp_c) masked.
__global__ void mix_loo_var_kernel(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                                   const double *m, const double *v, const double *ell, const double *L, const double *mean,
                                   double *var, int first) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows * d) return;
    const int64_t r = e / d;
    const int j = (int)(e - r * d);
    const double lp = logpost[r * nm + c];
    const double wgt = __builtin_isfinite(X[r * ldx + j]) ? exp(lp - ell[e] - L[e]) : exp(lp);
    const double dv = m[e] - mean[e];
    const double term = wgt * fma(dv, dv, v[e]);
    var[e] = first ? term : var[e] + term;
}

unsigned elem_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t loo_lds_bytes(int k) {
    const int kq = pad16(k);
    return sizeof(double) * ((size_t)k * kq + kq + 4);
}

hipError_t launch_loo(const double *X, int64_t ldx, int d, int k, int64_t n_rows, const double *model, const double *states,
                      const double *covs, double *mean, double *var, double *ell, double *llks, int n_cu, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const size_t lds = loo_lds_bytes(k);
    LooArgs a{X, ldx, d, k, n_rows, model, states, covs, mean, var, ell, llks};
    const int64_t grid = std::min<int64_t>(n_rows, (int64_t)std::max(n_cu, 1) * 8);
    if (hipError_t e = lds > 64 * 1024 ? ensure_dynamic_lds<loo_kernel>(lds) : hipSuccess; e != hipSuccess) return e;
    hipLaunchKernelGGL(loo_kernel, dim3((unsigned)grid), dim3(LOO_THREADS), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_mix_loo_fold(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                               const double *m, const double *ell, double *mx, double *sm, double *wm, int first, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(mix_loo_fold_kernel, dim3(elem_blocks(n_rows * d)), dim3(256), 0, s, X, ldx, d, n_rows, logpost, c, nm, m, ell,
                       mx, sm, wm, first);
    return hipGetLastError();
}

hipError_t launch_mix_loo_finish(const double *X, int64_t ldx, int d, int64_t n_rows, double *mx, const double *sm, const double *wm,
                                 double *mean, double *llks, int n_cu, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const int64_t grid = std::min<int64_t>(n_rows, (int64_t)std::max(n_cu, 1) * 8);
    hipLaunchKernelGGL(mix_loo_finish_kernel, dim3((unsigned)grid), dim3(LOO_THREADS), 0, s, X, ldx, d, n_rows, mx, sm, wm, mean,
                       llks);
    return hipGetLastError();
}

hipError_t launch_mix_loo_var(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                              const double *m, const double *v, const double *ell, const double *L, const double *mean, double *var,
                              int first, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(mix_loo_var_kernel, dim3(elem_blocks(n_rows * d)), dim3(256), 0, s, X, ldx, d, n_rows, logpost, c, nm, m, v,
                       ell, L, mean, var, first);
    return hipGetLastError();
}

}  // namespace ppca
