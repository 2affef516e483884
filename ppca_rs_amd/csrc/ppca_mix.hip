// ppca_mix.hip -- the mixture's helper kernels, each with its launcher below it: the posteriors and log
// posteriors of the components (one launch per stage for all components: mix_posteriors2 / mix_stage2), the two-stage max / sum
// reductions, the responsibility-sparse row selection of a component's pass (select_*, single and multi), the shifts and new
// log-weights, and the posterior-weighted accumulation of the outputs.  Small streaming kernels: none is templated on the state size.
#include "ppca_internal.hpp"

namespace ppca {

// mix.rs:283-295 (log-softmax of llk_c + log pi_c) and :304-309 (ln w_i + log posterior)
__global__ void mix_posteriors_kernel(const double *llk, const double *logw, const double *w, int64_t n, int nm,
                                      double *u, double *lse, double *logpost) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double mx = -INFINITY;
    for (int c = 0; c < nm; ++c) mx = fmax(mx, llk[(int64_t)c * n + i] + logw[c]);
    double s = 0.0;
    for (int c = 0; c < nm; ++c) s += exp(llk[(int64_t)c * n + i] + logw[c] - mx);
    const double ln = log(s);
    if (lse) lse[i] = mx + ln;
    const double wi = w ? w[i] : 1.0;
    const double lw = wi > 0.0 ? log(wi) : -INFINITY;
    for (int c = 0; c < nm; ++c) {
        double lp = llk[(int64_t)c * n + i] + logw[c] - mx - ln;
        if (logpost) logpost[i * nm + c] = lp;
        if (u) u[(int64_t)c * n + i] = lw + lp;
    }
}
hipError_t launch_mix_posteriors(const double *llk, const double *logw_dev, const double *w, int64_t n, int nm,
                                 double *u, double *lse, double *logpost, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mix_posteriors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, llk, logw_dev, w, n,
                       nm, u, lse, logpost);
    return hipGetLastError();
}

// The same + what the mixture step needs of u and lse afterwards, so that no further sweep over them is launched: per block of 256
// samples the maxima of u_c (NaNs skipped, mix.rs:312-315) and the sum of w_i lse_i, into bpart[nm + 1][gridDim.x] (fixed order: lane
// butterflies, then the four waves in index order).  nm <= MIX_MAX.
__global__ __launch_bounds__(256) void mix_posteriors2_kernel(const double *llk, const double *logw, const double *w, int64_t n, int nm,
                                                               double *u, double *lse, double *bpart) {
    __shared__ double red[4][MIX_MAX + 1];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    double lv[MIX_MAX], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < MIX_MAX; ++c) {
        lv[c] = (in && c < nm) ? llk[(int64_t)c * n + i] + logw[c] : -INFINITY;
        if (c < nm) mx = fmax(mx, lv[c]);
    }
    double sm = 0.0;
#pragma unroll
    for (int c = 0; c < MIX_MAX; ++c)
        if (c < nm) sm += exp(lv[c] - mx);
    const double ln = log(sm);
    const double wi = in ? (w ? w[i] : 1.0) : 0.0;
    const double lw = wi > 0.0 ? log(wi) : -INFINITY;
    if (in) lse[i] = mx + ln;
    double part = in ? (w ? (mx + ln) * wi : mx + ln) : 0.0;  // (launch_reduce_sum's term: v w or v)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) red[wave][MIX_MAX] = part;
#pragma unroll
    for (int c = 0; c < MIX_MAX; ++c) {
        if (c < nm) {
            double uc = -INFINITY;
            if (in) {
                const double v = lw + (lv[c] - mx - ln);
                u[(int64_t)c * n + i] = v;
                uc = (v == v) ? v : -INFINITY;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) uc = fmax(uc, __shfl_xor(uc, o, 64));
            if (lane == 0) red[wave][c] = uc;
        }
    }
    __syncthreads();
    if (threadIdx.x < nm) {
        const int c = threadIdx.x;
        bpart[(int64_t)c * gridDim.x + blockIdx.x] = fmax(fmax(red[0][c], red[1][c]), fmax(red[2][c], red[3][c]));
    } else if (threadIdx.x == MIX_MAX) {
        bpart[(int64_t)nm * gridDim.x + blockIdx.x] = (red[0][MIX_MAX] + red[1][MIX_MAX]) + (red[2][MIX_MAX] + red[3][MIX_MAX]);
    }
}
hipError_t launch_mix_posteriors2(const double *llk, const double *logw_dev, const double *w, int64_t n, int nm, double *u, double *lse,
                                  double *bpart, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (nm > MIX_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mix_posteriors2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, llk, logw_dev, w, n, nm, u, lse, bpart);
    return hipGetLastError();
}
// Second stage: workgroup c < nm: maxima[c] = max of bpart[c][0 .. nb); workgroup nm: *llk_out = sum of bpart[nm][0 .. nb) -- thread t
// takes the blocks t, t + 256, ... in order, then a fixed tree.
__global__ __launch_bounds__(256) void mix_stage2_kernel(const double *bpart, int nb, int nm, double *maxima, double *llk_out) {
    __shared__ double red[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const bool is_max = c < nm;
    double acc = is_max ? -INFINITY : 0.0;
    for (int b = t; b < nb; b += 256) {
        const double v = bpart[(int64_t)c * nb + b];
        acc = is_max ? fmax(acc, v) : acc + v;
    }
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = is_max ? fmax(red[t], red[t + o]) : red[t] + red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        if (is_max) maxima[c] = red[0];
        else *llk_out = red[0];
    }
}
hipError_t launch_mix_stage2(const double *bpart, int64_t n, int nm, double *maxima, double *llk_out, hipStream_t s) {
    const int nb = (int)((n + 255) / 256);
    hipLaunchKernelGGL(mix_stage2_kernel, dim3(nm + 1), dim3(256), 0, s, bpart, nb, nm, maxima, llk_out);
    return hipGetLastError();
}

template <bool MAX>
__global__ void reduce_stage_kernel(const double *v, const double *w, int64_t n, double *out, const int *n_dev = nullptr) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if (n_dev) n = *n_dev;  // (the count was produced on the device; the grid is sized for an upper bound)
    double acc = MAX ? -INFINITY : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        double x = v[i];
        if (MAX) {
            if (x == x) acc = fmax(acc, x);  // NaNs are skipped (mix.rs:312-315)
        } else {
            acc += w ? x * w[i] : x;
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = MAX ? fmax(red[tid], red[tid + o]) : red[tid] + red[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}
// two-stage deterministic reductions; work must hold >= 1024 doubles
hipError_t launch_reduce_max(const double *v, int64_t n, double *out_scalar, double *work, hipStream_t s) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((reduce_stage_kernel<true>), dim3(blocks), dim3(256), 0, s, v, (const double *)nullptr, n, work, (const int *)nullptr);
    hipLaunchKernelGGL((reduce_stage_kernel<true>), dim3(1), dim3(256), 0, s, work, (const double *)nullptr,
                       (int64_t)blocks, out_scalar, (const int *)nullptr);
    return hipGetLastError();
}
hipError_t launch_reduce_sum(const double *v, const double *w, int64_t n, double *out_scalar, double *work,
                             hipStream_t s, const int *n_dev) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((reduce_stage_kernel<false>), dim3(blocks), dim3(256), 0, s, v, w, n, work, n_dev);
    hipLaunchKernelGGL((reduce_stage_kernel<false>), dim3(1), dim3(256), 0, s, work, (const double *)nullptr,
                       (int64_t)blocks, out_scalar, (const int *)nullptr);
    return hipGetLastError();
}

__global__ void exp_shift_kernel(const double *v, const double *mx, int64_t n, double *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = exp(v[i] - *mx);
}
hipError_t launch_exp_shift(const double *v, const double *max_dev, int64_t n, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(exp_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, max_dev, n, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ responsibility-sparse component passes
// Per mixture component the sample weights are exp(u_i - max) (mix.rs:320-323): the largest is exactly 1.  Every
// statistic is a sum of weight x per-sample term, so a sample whose weight is below 2^-200 (6e-61) of the largest
// moves no statistic: its term is >= 147 binary orders below the fp64 resolution of the sum it would join (the
// exponential underflows to exactly zero only past 2^-1074; at d = 256 most samples of the other clusters sit far
// below either bound).  Such samples are dropped from the component's pass.
// select_*: ascending list of the rows with a non-zero weight and their weights, in three deterministic steps
// (per-block counts, exclusive scan of the counts, ordered scatter); the EM pass then gathers those rows.
constexpr int SEL_BLOCK = 256;
constexpr double SEL_MIN_WEIGHT = 6.223015277861142e-61;  // 2^-200
__global__ __launch_bounds__(SEL_BLOCK) void select_count_kernel(const double *v, const double *shift, int64_t n, int *counts) {
    const int64_t i = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool keep = i < n && exp(v[i] - *shift) > SEL_MIN_WEIGHT;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
    __shared__ int wc[SEL_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
// counts[0 .. nblocks) -> exclusive offsets in place; counts[nblocks] = total.  One workgroup.
__global__ __launch_bounds__(1024) void select_scan_kernel(int *counts, int nblocks) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int b0 = t * per, b1 = (b0 + per < nblocks) ? b0 + per : nblocks;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += counts[b];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan of the per-thread sums
        const int add = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = b0; b < b1; ++b) {
        const int c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (t == 1023) counts[nblocks] = part[1023];
}
__global__ __launch_bounds__(SEL_BLOCK) void select_scatter_kernel(const double *v, const double *shift, int64_t n,
                                                                    const int *offsets, int *rows, double *wout) {
    const int64_t i = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const double w = i < n ? exp(v[i] - *shift) : 0.0;
    const bool keep = w > SEL_MIN_WEIGHT;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
    __shared__ int wc[SEL_BLOCK / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wc[wave] = __popcll(bal);
    __syncthreads();
    int base = offsets[blockIdx.x];
    for (int u = 0; u < wave; ++u) base += wc[u];
    if (keep) {
        const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        rows[pos] = (int)i;
        wout[pos] = w;
    }
}
hipError_t launch_select_positive(const double *v, const double *shift_dev, int64_t n, int *counts, int *rows, double *wout,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int nblocks = (int)((n + SEL_BLOCK - 1) / SEL_BLOCK);
    hipLaunchKernelGGL(select_count_kernel, dim3(nblocks), dim3(SEL_BLOCK), 0, s, v, shift_dev, n, counts);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(1024), 0, s, counts, nblocks);
    hipLaunchKernelGGL(select_scatter_kernel, dim3(nblocks), dim3(SEL_BLOCK), 0, s, v, shift_dev, n, counts, rows, wout);
    return hipGetLastError();
}
int select_blocks(int64_t n) { return (int)((n + SEL_BLOCK - 1) / SEL_BLOCK); }

// The three selection steps for nm components at once (blockIdx.y = component; component c's arrays at c * n, its counts at
// c * (nb + 1)), the scatter also leaving the block's sum of kept weights (fixed order), and a last step that sums those per component.
__global__ __launch_bounds__(SEL_BLOCK) void select_count_multi_kernel(const double *u, const double *shift, int64_t n, int nb, int *counts) {
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const bool keep = i < n && exp(u[(int64_t)c * n + i] - shift[c]) > SEL_MIN_WEIGHT;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
    __shared__ int wc[SEL_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) counts[(int64_t)c * (nb + 1) + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
__global__ __launch_bounds__(1024) void select_scan_multi_kernel(int *counts_all, int nblocks) {
    int *counts = counts_all + (int64_t)blockIdx.x * (nblocks + 1);
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (nblocks + 1023) / 1024;
    const int b0 = t * per, b1 = (b0 + per < nblocks) ? b0 + per : nblocks;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += counts[b];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int add = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = b0; b < b1; ++b) {
        const int c = counts[b];
        counts[b] = run;
        run += c;
    }
    if (t == 1023) counts[nblocks] = part[1023];
}
__global__ __launch_bounds__(SEL_BLOCK) void select_scatter_multi_kernel(const double *u, const double *shift, int64_t n, int nb, const int *counts,
                                                                          int *rows, double *wout, double *wpart) {
    const int c = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const double w = i < n ? exp(u[(int64_t)c * n + i] - shift[c]) : 0.0;
    const bool keep = w > SEL_MIN_WEIGHT;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
    __shared__ int wc[SEL_BLOCK / 64];
    __shared__ double ws[SEL_BLOCK / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double sw = keep ? w : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sw += __shfl_xor(sw, o, 64);
    if (lane == 0) {
        wc[wave] = __popcll(bal);
        ws[wave] = sw;
    }
    __syncthreads();
    int base = counts[(int64_t)c * (nb + 1) + blockIdx.x];
    for (int q = 0; q < wave; ++q) base += wc[q];
    if (keep) {
        const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        rows[(int64_t)c * n + pos] = (int)i;
        wout[(int64_t)c * n + pos] = w;
    }
    if (threadIdx.x == 0) wpart[(int64_t)c * nb + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
__global__ __launch_bounds__(256) void mix_wsum_kernel(const double *wpart, int nb, const int *counts, double *sums_out, int *used_out) {
    __shared__ double red[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double acc = 0.0;
    for (int b = t; b < nb; b += 256) acc += wpart[(int64_t)c * nb + b];
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        sums_out[c] = red[0];
        used_out[c] = counts[(int64_t)c * (nb + 1) + nb];
    }
}
hipError_t launch_select_multi(const double *u, const double *shift_dev, int64_t n, int nm, int *counts, int *rows, double *wout, double *wpart,
                               double *sums_out, int *used_out, hipStream_t s) {
    if (n <= 0 || nm <= 0) return hipSuccess;
    const int nb = (int)((n + SEL_BLOCK - 1) / SEL_BLOCK);
    hipLaunchKernelGGL(select_count_multi_kernel, dim3(nb, nm), dim3(SEL_BLOCK), 0, s, u, shift_dev, n, nb, counts);
    hipLaunchKernelGGL(select_scan_multi_kernel, dim3(nm), dim3(1024), 0, s, counts, nb);
    hipLaunchKernelGGL(select_scatter_multi_kernel, dim3(nb, nm), dim3(SEL_BLOCK), 0, s, u, shift_dev, n, nb, (const int *)counts, rows, wout, wpart);
    hipLaunchKernelGGL(mix_wsum_kernel, dim3(nm), dim3(256), 0, s, (const double *)wpart, nb, (const int *)counts, sums_out, used_out);
    return hipGetLastError();
}

// shifts of the mixture's component weights (mix.rs:312-323): a maximum that is not finite (no sample with a finite
// ln w + log r: an empty shard set, or all weights zero) becomes 0 -- on the device, after the all-reduce(MAX)
__global__ void mix_shift_kernel(double *mx, int nm) {
    for (int c = threadIdx.x; c < nm; c += blockDim.x) {
        const double v = mx[c];
        mx[c] = (v - v == 0.0) ? v : 0.0;
    }
}
hipError_t launch_mix_shift(double *mx, int nm, hipStream_t s) {
    hipLaunchKernelGGL(mix_shift_kernel, dim3(1), dim3(256), 0, s, mx, nm);
    return hipGetLastError();
}
// new log-weights (mix.rs:324-325, :335): logsum_c = ln(sum_c) + shift_c, then robust_log_softmax (mix.rs:14-18); one
// workgroup; out[0 .. nm) the log-weights, out[nm] = *llk (so that ONE copy brings both to the host).  Any number of
// components: out[] itself holds the logsums between the two sweeps.
__global__ void mix_logweights_kernel(const double *sums, const double *shift, const double *llk, int nm, double *out) {
    __shared__ double red[2];
    const int t = threadIdx.x;
    for (int c = t; c < nm; c += blockDim.x) out[c] = log(sums[c]) + shift[c];
    __syncthreads();
    if (t == 0) {  // (one thread, index order: the result does not depend on the launch shape)
        double mx = -INFINITY;
        for (int i = 0; i < nm; ++i) mx = fmax(mx, out[i]);
        double sm = 0.0;
        for (int i = 0; i < nm; ++i) sm += exp(out[i] - mx);
        red[0] = mx;
        red[1] = log(sm);
        out[nm] = llk ? *llk : 0.0;
    }
    __syncthreads();
    const double mx = red[0], ln = red[1];
    for (int c = t; c < nm; c += blockDim.x) out[c] = out[c] - mx - ln;
}
hipError_t launch_mix_logweights(const double *sums, const double *shift, const double *llk, int nm, double *out, hipStream_t s) {
    hipLaunchKernelGGL(mix_logweights_kernel, dim3(1), dim3(256), 0, s, sums, shift, llk, nm, out);
    return hipGetLastError();
}
// Posterior-weighted accumulation over mixture components (mix.rs:404-423, :447-461, :489-505):
//   out (first ? = : +=) exp(logpost[i][c]) * (dev ? a + (dev - mean)^2 : a)
__global__ void mix_accumulate_kernel(double *out, const double *a, const double *dev, const double *mean,
                                      const double *logpost, int c, int nm, int64_t n, int d, int first) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * d) return;
    const int64_t i = idx / d;
    const double wgt = exp(logpost[i * nm + c]);
    double v = a[idx];
    if (dev) {
        const double t = dev[idx] - mean[idx];
        v += t * t;
    }
    out[idx] = first ? wgt * v : out[idx] + wgt * v;
}
hipError_t launch_mix_accumulate(double *out, const double *a, const double *dev, const double *mean,
                                 const double *logpost, int c, int nm, int64_t n, int d, int first, hipStream_t s) {
    if (n <= 0 || d <= 0) return hipSuccess;
    hipLaunchKernelGGL(mix_accumulate_kernel, dim3((unsigned)((n * d + 255) / 256)), dim3(256), 0, s, out, a, dev, mean,
                       logpost, c, nm, n, d, first);
    return hipGetLastError();
}

}  // namespace ppca
