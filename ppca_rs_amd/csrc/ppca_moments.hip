// ppca_moments.hip -- the pairwise second moments of a masked dataset: for an N x d dataset with row
// weights w, a per-column centre b and x~_ij = x_ij - b_j on observed entries (0 on masked ones), three d x d matrices
//
//   sums[j][l]   = sum_i w_i x~_ij x~_il      (rows where both are observed)                      symmetric
//   counts[j][l] = sum_i w_i m_ij m_il                                                            symmetric
//   cross[j][l]  = sum_i w_i x~_ij m_il       (centred column j over the rows where l is observed)   only when asked for
//
// These are the dense contractions X~^T diag(w) X~, M^T diag(w) M and X~^T diag(w) M (d x N times N x d) on v_mfma_f64_16x16x4_f64:
// one f64 of A and one of B per lane, C/D col = lane & 15, row = (lane >> 4) + 4 reg.  The columns are cut into tiles of 64; a
// job is a tile pair (I <= J) x a run of rows.  Per step of 16 rows the workgroup stages the row panel of column tile I and of
// tile J (only one when I = J) in LDS as two planes each -- x~ with the centring and the mask already applied BY SELECTION (a
// masked entry is stored as 0.0, never multiplied away: a NaN times 0 is a NaN) and m as 1.0 / 0.0 -- plus the 16 weights (in the
// padding of the rows); wave w owns rows 16 w .. 16 w + 15 of the 64 x 64 tile and all four 16-column blocks.  The weight goes on
// the A operand (w x~ one rounding, w m by selection), so that with no weights or integer ones `counts` is an exact integer sum.
// With `cross` a pair also
// computes (w x~_I)^T M_J = cross[I][J] and, when I < J, (w M_I)^T X~_J = the transpose of cross[J][I]: four products where the
// symmetric pair takes two.  The next step's panel is fetched into registers before the MFMAs of the current one.
//
// Each job writes its 64 x 64 partials (2, or 4 with `cross`) to scratch; moments_reduce_kernel then adds the row runs of every
// output element in run order and writes the upper triangle of `sums` and `counts` to both (j, l) and (l, j) -- also inside the
// diagonal tiles, whose two MFMA triangles round differently -- so that both are symmetric bit for bit.  No float atomics: the
// result is bit-reproducible for a given grid.  The number of row runs comes from the context's workgroup count
// (MOMENTS_WG_PER_CU workgroups per CU over the tile pairs), each run a multiple of 16 rows.
//
// Scratch: jobs x (2 or 4) x 32 KiB with jobs <= MOMENTS_WG_PER_CU x workgroups + T (T + 1) / 2, T = ceil(d / 64): independent of N
// (256 CUs, d = 256: 1546 jobs, 97 MiB; 193 MiB with cross).
#include <algorithm>

#include "ppca_internal.hpp"

namespace ppca {
namespace {

typedef double d4m_t __attribute__((ext_vector_type(4)));

constexpr int MT = 64;        // column tile
constexpr int MR = 16;        // rows per step
constexpr int MLD = 80;       // LDS row stride in doubles: 640 B puts the four row quarters of a wave's read on disjoint bank halves;
                              // column MT of plane 0 of Xs holds the row's weight (40 KiB in all)
constexpr int MOMENTS_WG_PER_CU = 6;  // jobs per CU: 164 registers without cross (three workgroups resident per CU), 214 with (two)

struct MomentsArgs {
    const double *X;
    int64_t ldx, n;
    int d;
    const double *w;       // nullable (= 1)
    const double *center;  // d
    int tiles, npairs, nsplit;
    int64_t rows_per;      // rows of a run (a multiple of MR)
    double *part;          // [nsplit][npairs][nq][64][64]
};

// pair index p -> (I, J), I <= J, row by row of the upper triangle
__device__ __host__ inline void pair_of(int p, int tiles, int *I, int *J) {
    int i = 0;
    while (p >= tiles - i) {
        p -= tiles - i;
        ++i;
    }
    *I = i;
    *J = i + p;
}
__device__ __host__ inline int pair_index(int I, int J, int tiles) { return I * tiles - I * (I - 1) / 2 + (J - I); }

template <bool CROSS>
__global__ __launch_bounds__(256) void moments_kernel(MomentsArgs a) {
    __shared__ double Xs[2][MR][MLD];
    __shared__ double Ms[2][MR][MLD];
    constexpr int NQ = CROSS ? 4 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int pair = (int)(blockIdx.x % (unsigned)a.npairs), split = (int)(blockIdx.x / (unsigned)a.npairs);
    int I, J;
    pair_of(pair, a.tiles, &I, &J);
    const bool diag = I == J;
    const int pj = diag ? 0 : 1;  // the plane the B operands come from
    const int64_t r0 = (int64_t)split * a.rows_per, r1 = r0 + a.rows_per < a.n ? r0 + a.rows_per : a.n;

    d4m_t acc[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] = d4m_t{0, 0, 0, 0};

    // staging: thread -> row tid / 16 of the step, four consecutive columns of each panel.  Every load is unconditional on a
    // clamped address and the validity is a select afterwards.
    const int sr = tid >> 4, sc = (tid & 15) * 4;
    int col[2][4];
    bool cok[2][4];
    double cen[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = (p == 0 ? I : J) * MT + sc + u;
            cok[p][u] = c < a.d;
            col[p][u] = cok[p][u] ? c : a.d - 1;
            cen[p][u] = a.center[col[p][u]];
        }
    double rx[2][4], rw = 0.0;
    bool rok = false;
    auto fetch = [&](int64_t rb) {
        const int64_t r = rb + sr;
        rok = r < r1;
        const int64_t rc = rok ? r : r1 - 1;  // (r0 < r1 for every job)
        const double *row = a.X + rc * a.ldx;
#pragma unroll
        for (int u = 0; u < 4; ++u) rx[0][u] = row[col[0][u]];
        if (!diag)
#pragma unroll
            for (int u = 0; u < 4; ++u) rx[1][u] = row[col[1][u]];
        rw = a.w ? a.w[rc] : 1.0;
    };
    auto stash = [&]() {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p == 1 && diag) break;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool obs = rok && cok[p][u] && __builtin_isfinite(rx[p][u]);
                Xs[p][sr][sc + u] = obs ? __dsub_rn(rx[p][u], cen[p][u]) : 0.0;  // select, never multiply
                Ms[p][sr][sc + u] = obs ? 1.0 : 0.0;
            }
        }
        if ((tid & 15) == 0) Xs[0][sr][MT] = rok ? rw : 0.0;
    };

    fetch(r0);
    for (int64_t rb = r0; rb < r1; rb += MR) {
        stash();
        __syncthreads();
        if (rb + MR < r1) fetch(rb + MR);
#pragma unroll
        for (int s = 0; s < MR / 4; ++s) {
            const int k = 4 * s + l4;
            const double wv = Xs[0][k][MT];
            const bool ob = Ms[0][k][16 * wave + l15] != 0.0;  // (the weight by selection too, as scale_kernel takes it)
            const double ax = ob ? __dmul_rn(Xs[0][k][16 * wave + l15], wv) : 0.0;
            const double am = ob ? wv : 0.0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double bx = Xs[pj][k][16 * t + l15], bm = Ms[pj][k][16 * t + l15];
                acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bx, acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bm, acc[1][t], 0, 0, 0);
                if constexpr (CROSS) {
                    acc[2][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bm, acc[2][t], 0, 0, 0);
                    if (!diag) acc[3][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bx, acc[3][t], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // the whole 64 x 64 tile of every product goes out, tail rows and columns included (they are zeros): the scratch is dense
    double *out = a.part + ((int64_t)split * a.npairs + pair) * NQ * (MT * MT);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(q * MT + 16 * wave + l4 + 4 * r) * MT + 16 * t + l15] = acc[q][t][r];
}

// One thread per element (j, l) of the d x d outputs: the row runs in run order.  sums / counts: the threads of the upper triangle
// write both (j, l) and (l, j); cross: every thread writes its own element, from product 2 of the pair (tile j, tile l) when
// tile j <= tile l, else from product 3 of the pair (tile l, tile j), which holds the transpose.
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double *part, int d, int tiles, int npairs, int nsplit, int nq,
                                                             double *sums, double *counts, double *cross) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)d * d) return;
    const int j = (int)(idx / d), l = (int)(idx - (int64_t)j * d);
    const int tj = j / MT, tl = l / MT, jj = j - tj * MT, ll = l - tl * MT;
    const int64_t stride = (int64_t)npairs * nq * (MT * MT);
    if (j <= l) {
        const double *p = part + (int64_t)pair_index(tj, tl, tiles) * nq * (MT * MT) + jj * MT + ll;
        double s = 0.0, c = 0.0;
        for (int r = 0; r < nsplit; ++r) {
            s += p[r * stride];
            c += p[r * stride + MT * MT];
        }
        sums[(int64_t)j * d + l] = s;
        sums[(int64_t)l * d + j] = s;
        counts[(int64_t)j * d + l] = c;
        counts[(int64_t)l * d + j] = c;
    }
    if (cross) {
        const double *p = tj <= tl ? part + ((int64_t)pair_index(tj, tl, tiles) * nq + 2) * (MT * MT) + jj * MT + ll
                                   : part + ((int64_t)pair_index(tl, tj, tiles) * nq + 3) * (MT * MT) + ll * MT + jj;
        double x = 0.0;
        for (int r = 0; r < nsplit; ++r) x += p[r * stride];
        cross[(int64_t)j * d + l] = x;
    }
}

}  // namespace

MomentsPlan moments_plan(int64_t n, int d, int n_cu, bool cross) {
    MomentsPlan p{};
    p.tiles = (d + MT - 1) / MT;
    p.npairs = p.tiles * (p.tiles + 1) / 2;
    p.nq = cross ? 4 : 2;
    if (n <= 0) return p;  // (nsplit = 0: nothing to launch)
    const int64_t want = std::max<int64_t>(1, ((int64_t)std::max(n_cu, 1) * MOMENTS_WG_PER_CU + p.npairs - 1) / p.npairs);
    const int64_t per = (n + want - 1) / want;
    p.rows_per = (per + MR - 1) / MR * MR;
    p.nsplit = (int)((n + p.rows_per - 1) / p.rows_per);
    p.scratch_bytes = sizeof(double) * (size_t)p.nsplit * p.npairs * p.nq * (MT * MT);
    return p;
}

hipError_t launch_pairwise_moments(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *center_dev,
                                   const MomentsPlan &p, double *part, double *sums, double *counts, double *cross, hipStream_t s) {
    if (n <= 0 || p.nsplit <= 0) return hipSuccess;
    MomentsArgs a{X, ldx, n, d, w, center_dev, p.tiles, p.npairs, p.nsplit, p.rows_per, part};
    const dim3 g((unsigned)((int64_t)p.nsplit * p.npairs)), b(256);
    if (cross)
        hipLaunchKernelGGL(moments_kernel<true>, g, b, 0, s, a);
    else
        hipLaunchKernelGGL(moments_kernel<false>, g, b, 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int64_t total = (int64_t)d * d;
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, d, p.tiles, p.npairs, p.nsplit,
                       p.nq, sums, counts, cross);
    return hipGetLastError();
}

}  // namespace ppca
