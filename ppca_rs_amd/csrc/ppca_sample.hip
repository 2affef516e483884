// ppca_sample.hip -- posterior sampling and multiple imputation on the device (ppca_posterior_sample,
// ppca_mix_posterior_sample).
//
// The draw of row i (global row g = row_offset + i) with posterior mean z_i and covariance Sigma_i (what ppca_infer returns):
//     U_i  upper triangular, positive diagonal, Sigma_i = U_i U_i^T (the reverse-order Cholesky of Sigma_i; = sigma L_i^-T
//          for the lower Cholesky factor L_i of M_i = C_o^T C_o + sigma^2 I)
//     x_i  = C (z_i + U_i eps_i) + mean + sigma eta_i                       mode 0 (sample, ppca_model.rs:597-626)
//     x_ij = the input where it is observed, the mode-0 value elsewhere     mode 1 (one draw of multiple imputation)
// eps_i in R^k, eta_i in R^d are standard normals of the counter-based generator of ppca_sweep.hpp (streams STREAM_EPS,
// STREAM_ETA; the mixture's component: STREAM_CHOICE), keyed by (seed, stream, g, index): nothing depends on the grid, the chunking
// of the rows or the path that produced z_i and Sigma_i.  DESIGN.md section 4.9 states the generator;
// tests/test_gpu_posterior_sample.py restates it bit for bit.
#include <algorithm>

#include "ppca_sweep.hpp"

namespace ppca {
namespace {

// Box-Muller on both branches of one word (one finaliser per PAIR of normals), fp32: u1 = (top 24 bits + 1) 2^-24 in (0, 1],
// u2 = (bits 16..39) 2^-24 in [0, 1)
__device__ __forceinline__ void normal_pair(uint64_t w, double &n0, double &n1) {
    const float u1 = (float)((w >> 40) + 1ull) * 5.9604644775390625e-08f;
    const float u2 = (float)((w >> 16) & 0xFFFFFFull) * 5.9604644775390625e-08f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    n0 = (double)(r * c);
    n1 = (double)(r * s);
}

struct DrawArgs {
    const double *X;       // input rows (masks, and the observed values of mode 1)
    int64_t ldx;
    int d, k;              // k: the model's kernel state size (a state size 0 runs as one zero column)
    int64_t n_rows;        // rows of this chunk
    int64_t row0;          // first row of the chunk within the dataset
    int64_t row_offset;    // + row0 + r = the row's key
    const double *model;   // [sigma, sigma^2, ln sigma, 0 | C (d x k) | mean (d)]
    const double *states;  // chunk (n_rows x k)
    const double *covs;    // chunk (n_rows x k x k)
    double *out;           // whole output (dataset rows x d)
    int mode;
    uint64_t seed;
    const int *choice;     // nullable: only rows whose choice[row] == comp are written (the mixture)
    int comp;
};

// One wave per row (grid-stride over the chunk).  LDS: the index-reversed Sigma, lower-packed (k(k+1)/2), eps (k), z + U eps (k).
__global__ __launch_bounds__(64) void posterior_draw_kernel(DrawArgs a) {
    extern __shared__ double lds[];
    const int k = a.k, d = a.d, lane = threadIdx.x;
    const int kp = k * (k + 1) / 2;
    double *A = lds, *E = lds + kp, *W = E + k;
    const double sigma = a.model[0];
    const double *C = a.model + 4;
    const double *mean = C + (int64_t)d * k;
    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t i = a.row0 + r;
        if (a.choice && a.choice[i] != a.comp) continue;  // (uniform over the block)
        const uint64_t g = (uint64_t)(a.row_offset + i);
        const double *S = a.covs + r * k * k;
        // A = P Sigma P (P reverses the index order), lower-packed: A[ii][jj] at ii(ii+1)/2 + jj
        for (int ii = 0; ii < k; ++ii)
            for (int jj = lane; jj <= ii; jj += 64) A[ii * (ii + 1) / 2 + jj] = S[(int64_t)(k - 1 - ii) * k + (k - 1 - jj)];
        const uint64_t ke = row_key(a.seed, STREAM_EPS, g);
        for (int p = lane; 2 * p < k; p += 64) {
            double n0, n1;
            normal_pair(row_word(ke, (uint64_t)p), n0, n1);
            E[2 * p] = n0;
            if (2 * p + 1 < k) E[2 * p + 1] = n1;
        }
        __syncthreads();
        // right-looking Cholesky A = L L^T in place; U = P L P.  A pivot that rounding took to <= 0 (Sigma of a model whose rows of C
        // span many orders of magnitude has eigenvalues below the rounding of its largest) gives a zero column: no spread in
        // a direction where the posterior has none to resolve
        for (int c = 0; c < k; ++c) {
            const double a = A[c * (c + 1) / 2 + c];
            const double piv = a > 0.0 ? sqrt(a) : 0.0;
            __syncthreads();
            for (int ii = c + 1 + lane; ii < k; ii += 64) A[ii * (ii + 1) / 2 + c] = piv > 0.0 ? A[ii * (ii + 1) / 2 + c] / piv : 0.0;
            if (lane == 0) A[c * (c + 1) / 2 + c] = piv;
            __syncthreads();
            for (int ii = c + 1; ii < k; ++ii) {
                const double lic = A[ii * (ii + 1) / 2 + c];
                for (int jj = c + 1 + lane; jj <= ii; jj += 64) A[ii * (ii + 1) / 2 + jj] -= lic * A[jj * (jj + 1) / 2 + c];
            }
            __syncthreads();
        }
        // W = z + U eps: (U eps)[k-1-ii] = sum_{jj <= ii} L[ii][jj] eps[k-1-jj]
        for (int ii = lane; ii < k; ii += 64) {
            double s = a.states[r * k + (k - 1 - ii)];
            for (int jj = 0; jj <= ii; ++jj) s += A[ii * (ii + 1) / 2 + jj] * E[k - 1 - jj];
            W[k - 1 - ii] = s;
        }
        __syncthreads();
        const uint64_t kh = row_key(a.seed, STREAM_ETA, g);
        const double *x = a.X + i * a.ldx;
        double *o = a.out + i * d;
        for (int p = lane; 2 * p < d; p += 64) {
            double nz[2];
            normal_pair(row_word(kh, (uint64_t)p), nz[0], nz[1]);
            for (int h = 0; h < 2; ++h) {
                const int j = 2 * p + h;
                if (j >= d) break;
                double v = mean[j] + sigma * nz[h];
                const double *cj = C + (int64_t)j * k;
                for (int b = 0; b < k; ++b) v += cj[b] * W[b];
                if (a.mode == 1) {
                    const double xv = x[j];
                    if (__builtin_isfinite(xv)) v = xv;
                }
                o[j] = v;
            }
        }
        __syncthreads();  // LDS is reused by the next row
    }
}

// The mixture's component per row: the first c with u < sum_{c' <= c} exp(logpost[i][c']), u the row's uniform of the choice
// stream; rounding past the last sum takes the last component of positive posterior.
__global__ void mix_choose_kernel(const double *logpost, int64_t n, int nm, uint64_t seed, int64_t row_offset, int *choice) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double u = u01_open(row_word(row_key(seed, STREAM_CHOICE, (uint64_t)(row_offset + i)), 0));
    double cum = 0.0;
    int pick = -1, last = 0;
    for (int c = 0; c < nm; ++c) {
        const double p = exp(logpost[i * nm + c]);
        if (p > 0.0) last = c;
        cum += p;
        if (pick < 0 && u < cum) pick = c;
    }
    choice[i] = pick >= 0 ? pick : last;
}

}  // namespace

size_t posterior_draw_lds_bytes(int k) { return sizeof(double) * ((size_t)k * (k + 1) / 2 + 2 * (size_t)k); }

hipError_t launch_posterior_draw(const double *X, int64_t ldx, int d, int k, int64_t n_rows, int64_t row0, int64_t row_offset,
                                 const double *model, const double *states, const double *covs, double *out, int mode,
                                 uint64_t seed, const int *choice, int comp, int n_cu, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    const size_t lds = posterior_draw_lds_bytes(k);
    if (hipError_t e = lds > 64 * 1024 ? ensure_dynamic_lds<posterior_draw_kernel>(lds) : hipSuccess; e != hipSuccess) return e;
    const int64_t grid = std::min<int64_t>(n_rows, (int64_t)std::max(n_cu, 1) * 32);
    DrawArgs a{X, ldx, d, k, n_rows, row0, row_offset, model, states, covs, out, mode, seed, choice, comp};
    hipLaunchKernelGGL(posterior_draw_kernel, dim3((unsigned)grid), dim3(64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_mix_choose(const double *logpost, int64_t n, int nm, uint64_t seed, int64_t row_offset, int *choice,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mix_choose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logpost, n, nm, seed, row_offset,
                       choice);
    return hipGetLastError();
}

}  // namespace ppca
