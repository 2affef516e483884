// ppca_util.hip -- the kernels around a dataset that no model family owns, each with its launcher below
// it: synthetic data, column presence, the canonical copy of masked entries, the row-scaling test hook, fill, and the two MFMA
// layout probes.
#include "ppca_sweep.hpp"

namespace ppca {

// ------------------------------------------------------------------ synthetic data
// (the generator and its streams: ppca_sweep.hpp)
__device__ __forceinline__ uint64_t rng_bits(uint64_t seed, uint64_t stream, uint64_t row, uint64_t col) {
    return row_word(row_key(seed, stream, row), col);
}
// fp64 Box-Muller from two words: not the draw of ppca_sample.hip's normal_pair
__device__ __forceinline__ double rng_normal(uint64_t seed, uint64_t stream, uint64_t row, uint64_t col) {
    double u1 = u01_open(rng_bits(seed, stream, row, 2 * col));
    double u2 = u01_open(rng_bits(seed, stream, row, 2 * col + 1));
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__global__ void synth_latent_kernel(double *z, int64_t row_offset, int64_t n_rows, int k, uint64_t seed) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * k) return;
    int64_t i = idx / k;
    int a = (int)(idx - i * k);
    z[idx] = rng_normal(seed, STREAM_SYNTH_LATENT, (uint64_t)(row_offset + i), (uint64_t)a);
}

__global__ void synth_data_kernel(const double *c, const double *mean, const double *z, double *x, int64_t row_offset,
                                  int64_t n_rows, int d, int k, double sigma, double mask_prob, int mask_kind,
                                  int mask_run, uint64_t seed) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * d) return;
    int64_t i = idx / d;
    int j = (int)(idx - i * d);
    const uint64_t grow = (uint64_t)(row_offset + i);
    double v = mean[j] + sigma * rng_normal(seed, STREAM_SYNTH_NOISE, grow, (uint64_t)j);
    for (int a = 0; a < k; ++a) v += c[(int64_t)j * k + a] * z[i * k + a];
    bool masked;
    if (mask_kind == 0) {
        masked = u01_open(rng_bits(seed, STREAM_SYNTH_MASK, grow, (uint64_t)j)) < mask_prob;
    } else {
        int start = (int)(u01_open(rng_bits(seed, STREAM_SYNTH_RUN, grow, 0)) * d);
        int off = j - start;
        if (off < 0) off += d;
        masked = off < mask_run;
    }
    x[idx] = masked ? __builtin_nan("") : v;
}
hipError_t launch_synth(const double *c_dev, const double *mean_dev, double *z_work, double *x_out, int64_t row_offset,
                        int64_t n_rows, int d, int k, double sigma, double mask_prob, int mask_kind, int mask_run,
                        uint64_t seed, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    int64_t nz = n_rows * k;
    if (nz > 0)
        hipLaunchKernelGGL(synth_latent_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, z_work, row_offset,
                           n_rows, k, seed);
    int64_t nx = n_rows * d;
    hipLaunchKernelGGL(synth_data_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, c_dev, mean_dev, z_work,
                       x_out, row_offset, n_rows, d, k, sigma, mask_prob, mask_kind, mask_run, seed);
    return hipGetLastError();
}

// present[j] = 1 if any sample has a finite value in dim j (Dataset::empty_dimensions, dataset.rs:194-222)
__global__ void column_presence_kernel(const double *X, int64_t ldx, int64_t n, int d, int *present) {
    int j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= d) return;
    int64_t rows_per = (n + gridDim.x - 1) / gridDim.x;
    int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
    int any = 0;
    for (int64_t r = r0; r < r1; ++r) any |= __builtin_isfinite(X[r * ldx + j]) ? 1 : 0;
    if (any) atomicOr(&present[j], 1);
}
hipError_t launch_column_presence(const double *X, int64_t ldx, int64_t n, int d, int *present, hipStream_t s) {
    if (n <= 0 || d <= 0) return hipSuccess;
    int gx = (int)((n + 4095) / 4096);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(column_presence_kernel, dim3(gx, (d + 255) / 256), dim3(256), 0, s, X, ldx, n, d, present);
    return hipGetLastError();
}

// dst[i] = src[i] if finite, NaN otherwise: masked entries leave the device in the canonical form of masked_vector
// (dataset.rs:64-72; +-inf inputs are masked, so they come back NaN too)
__global__ void canon_copy_kernel(const double *src, double *dst, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i + 1 < n) {
        typedef double d2_t __attribute__((ext_vector_type(2)));
        d2_t v = *reinterpret_cast<const d2_t *>(src + i);
        v[0] = __builtin_isfinite(v[0]) ? v[0] : __builtin_nan("");
        v[1] = __builtin_isfinite(v[1]) ? v[1] : __builtin_nan("");
        *reinterpret_cast<d2_t *>(dst + i) = v;
    } else if (i < n) {
        dst[i] = __builtin_isfinite(src[i]) ? src[i] : __builtin_nan("");
    }
}
hipError_t launch_canon_copy(const double *src, double *dst, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t pairs = (n + 1) / 2;
    hipLaunchKernelGGL(canon_copy_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}
// X[rows[i]][:] *= factor (bench / test hook: outlier rows in a device-resident dataset; non-finite entries stay masked)
__global__ void scale_rows_kernel(double *X, int64_t ldx, int d, const int64_t *rows, int64_t n_rows, double factor) {
    const int64_t i = blockIdx.x;
    if (i >= n_rows) return;
    for (int j = threadIdx.x; j < d; j += blockDim.x) X[rows[i] * ldx + j] *= factor;
}
hipError_t launch_scale_rows(double *X, int64_t ldx, int d, const int64_t *rows_dev, int64_t n_rows, double factor, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)n_rows), dim3(256), 0, s, X, ldx, d, rows_dev, n_rows, factor);
    return hipGetLastError();
}

__global__ void fill_kernel(double *p, int64_t n, double v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
hipError_t launch_fill(double *p, int64_t n, double v, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

__global__ void mfma_probe_kernel(const double *a, const double *b, double *out) {
    const int lane = threadIdx.x;
    d4_t acc = {0, 0, 0, 0};
    // A[i][kk] at lane = i + 16 kk ; B[kk][j] at lane = j + 16 kk
    acc = mfma(a[(lane & 15) * 4 + (lane >> 4)], b[(lane >> 4) * 16 + (lane & 15)], acc);
    for (int r = 0; r < 4; ++r) out[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
}
hipError_t launch_mfma_probe(const double *a16x4, const double *b4x16, double *out16x16, hipStream_t s) {
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, s, a16x4, b4x16, out16x16);
    return hipGetLastError();
}

// raw operand/result registers of one v_mfma_i32_16x16x64_i8: a, b: [64 lanes][16 bytes]; out: [64][4]
__global__ void mfma_i8_probe_kernel(const int *a, const int *b, int *out) {
    const int lane = threadIdx.x;
    i4_t av, bv, acc = {0, 0, 0, 0};
    for (int u = 0; u < 4; ++u) {
        av[u] = a[lane * 4 + u];
        bv[u] = b[lane * 4 + u];
    }
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc, 0, 0, 0);
    for (int u = 0; u < 4; ++u) out[lane * 4 + u] = acc[u];
}
hipError_t launch_mfma_i8_probe(const int *a, const int *b, int *out, hipStream_t s) {
    hipLaunchKernelGGL(mfma_i8_probe_kernel, dim3(1), dim3(64), 0, s, a, b, out);
    return hipGetLastError();
}

}  // namespace ppca
