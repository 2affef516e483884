// ppca_sparse.hip -- masked PPCA on row-compressed data (SparseDataset): the container, the host-side inverted
// index, the two passes that produce the packed statistics of include/ppca_hip.h from it, and the entry points that share the row
// pass (llk, infer, predict).  The model, the statistics buffer and the M-step are those of the dense path.
//
// Storage.  CSR on the device: row_ptr (int64, n + 1), col (int32, nnz, strictly increasing within a row), val (fp64, nnz).  Rows are
// cut into blocks of block_rows (fixed at construction: the records of a block stay under 1 GiB at k = 16).  Per block the host builds
//   - three row lists by row length m: m <= 16, m <= 64, longer (the bins of the row pass);
//   - the inverted index in CSC order (per column, the block's entries in ascending row): t_row (int32, row within the block) and
//     t_val, by a counting sort that is stable in row order (ppca_sparse_transpose_host);
//   - the work items of the column pass: a column with at most `segment` entries in the block is one item; a longer one is cut into
//     runs of exactly `segment` entries (the last one shorter), each an item that writes a partial.
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
//
// Held-out scoring (ppca_heldout_split_csr_host, ppca_heldout_score_sparse).  The split is host code: entry
// (g, j) draws the word of the dense split (ppca_heldout.hip) and is flagged held iff lo <= u < hi.  The score takes two datasets of
// equal n, d and block_rows, so that block b of `train` and block b of `held` cover the same rows.  Per block: sparse_row_kernel<K>
// writes z and Sigma of train's rows to scratch, then
// sparse_held_row_kernel<K>  runs over held's CSR with held's row lists and the groups of the row pass (W = 4 / 16 / 64 by the HELD
//     row's length).  Lane s takes the row's held entries s, s + W, ..., computes l of each (held_entry<K>: m, v by the k^2
//     multiply-adds of sparse_predict_kernel, in its order) and adds them in that order; one butterfly adds the lanes.  per_row of a
//     row depends on its train entry list (z, Sigma) and its held entry list alone.
// sparse_held_col_kernel<K>  runs over held's inverted index and work items.  An item belongs to a group of 16 lanes; lane s takes
//     the entries s, s + 16, ... of the item (ascending row), recomputes (m, v) from the row's (z, Sigma) with the same held_entry<K>
//     and forms [w | w l | w e^2 | w e^2 / v] (w: train's weight of the row).  Each chunk of 16 entries is added by one butterfly and
//     the chunks in order: a sum is a fixed function of the item's entry list.  A whole column adds into the 4 x d sums (blocks in
//     stream order); a run writes a partial and sparse_held_fix_kernel adds a column's runs in run order.  No float atomics.
//
// Top-n ranking (ppca_topn_sparse).  Per block: sparse_row_kernel<K> writes z (and Sigma when kappa != 0), then
// sparse_topn_kernel<K, VAR, R>  a wave takes a tile of R rows and a chunk of candidate positions and walks the chunk 64 at a time: a
//     lane holds c_j and mean_j of one column, z and Sigma of a row are wave-uniform, the score is sparse_predict_kernel's (mean, var)
//     multiply-add for multiply-add, and a row's list of n <= 64 (score, column) is held one entry per lane behind a wave-uniform
//     threshold.  The order (score descending, column ascending) is total, so the result depends on nothing else.
// sparse_topn_merge_kernel  when the columns were split into chunks: one wave per row offers the row's chunk lists in chunk order.
//
// The mixture (ppca_mix_sparse_llk / _em_step / _predict).
// sparse_mix_row_kernel<K, REG>  the row pass for up to MIX_MAX components of one state size: the row's entries fetched once (REG: kept
//     in registers across the components), ell_c into the component-major buffer of launch_mix_posteriors.  Its sums, tree,
//     factorisation and ell (sp_mix_row_ell) are sparse_row_kernel's operation for operation, so ell_c is sparse_row_kernel's bit for
//     bit; sparse_row_kernel itself is left as it was.  The step is ppca_host::mix_em_step's sequence with sp_accumulate under each
//     component's weight vector.
// sparse_mix_predict_kernel, sparse_mix_spread_kernel  the mixture predictive, component by component in index order per query entry.
//
// The mixture's top-n ranking (ppca_mix_topn_sparse).  The posteriors once; per block sparse_mix_resp_kernel
// (r = exp(log posterior)), sparse_row_kernel<k_c> per component into one scratch in the layout of the largest state size
// (sparse_pad_kernel for a smaller component), then
// sparse_mix_topn_kernel<K, VAR, R>  sparse_topn_kernel's work items, lists and windows with a loop over the components per 64 columns:
//     the score is fma(kappa, sqrt(var), mean) with sparse_mix_predict_kernel / sparse_mix_spread_kernel's (mean, var), operation for
//     operation; sparse_topn_merge_kernel when the columns were split.
//
// Factor analysis (ppca_scale_columns_sparse, ppca_fa_sparse_em_step).  A ppca_sparse may carry buffers of its
// own for the values in both orientations (a values view: the pattern, row lists, index and work items are the core's), and every
// launcher reads the values through the handle.
// sparse_scale_row_kernel  the CSR orientation, sparse_held_row_kernel's groups and bins: out_val = val * a[col] (one fp64 multiply)
//     and, optionally, the row's sum of l[col], lane s adding the entries s, s + W, ... in order, one butterfly.
// sparse_scale_col_kernel  the index orientation, sparse_held_col_kernel's items, 16-lane groups and runs: out_tval = tval * a_j (the
//     same multiply, the same bits) and, optionally, [sum w | sum w (x a_j - b_j) | sum w (x a_j - b_j)^2] per column: chunks of 16 by
//     butterfly, chunks in order, sparse_scale_fix_kernel adds a column's runs in run order.  No float atomics.
// The FA step whitens into a view, runs sp_accumulate on it under PPCAModel(1, C / s, mean / s) and hands the statistics to
// ppca_fa_finalize_host.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "ppca_handles.hpp"
#include "ppca_sweep.hpp"

using namespace ppca;
using namespace ppca_host;

namespace {

constexpr int SP_MAX_K = 16;
constexpr int SP_SHORT = 16, SP_MID = 64;  // row-length bins: W = 4, 16, 64
constexpr int SP_SEGMENT = 512;            // default run length of a long column
constexpr int SP_NSCAL = 5;                // per-row scalar terms: w sq_err | w dev | w ell | w | non-empty
constexpr int SP_SCAL_ROWS = 1024;         // rows per workgroup of sparse_scal_kernel

struct SpItem {
    int64_t start;  // first entry in t_row / t_val
    int64_t dest;   // < 0: add to the statistics; else the slot of the run's partial
    int32_t col, len;
};
struct SpLong {
    int64_t first;  // slot of the column's first run
    int32_t col, nruns;
};

struct SpBlock {
    int64_t row0 = 0, rows = 0, e0 = 0, nnz = 0;
    int64_t nbin[3] = {0, 0, 0}, bin_off[3] = {0, 0, 0};
    int64_t n_items = 0, n_long = 0, n_runs = 0;
    BufRef rowlist, items, longs;
};

struct SpCore {
    int64_t n = 0, nnz = 0, block_rows = 0, max_rows = 0, max_runs = 0, nonempty_rows = 0;
    int d = 0, segment = 0;
    BufRef row_ptr, col, val, trow, tval;
    std::vector<SpBlock> blocks;
    std::vector<int32_t> empty;  // 1 = column without an entry
    double build_seconds = 0.0;
};

}  // namespace

struct ppca_sparse {
    ppca_ctx *ctx = nullptr;
    std::shared_ptr<SpCore> core;
    BufRef wbuf;
    const double *w = nullptr;  // nullptr = all ones
    // A values view (ppca_scale_columns_sparse): buffers of its own for the values in CSR order and in
    // inverted-index order, on the pattern, row lists, index and work items of `core`.  Empty = the core's values.
    BufRef vbuf, tvbuf;
    const double *val() const { return static_cast<const double *>((vbuf ? vbuf : core->val)->p); }
    const double *tval() const { return static_cast<const double *>((tvbuf ? tvbuf : core->tval)->p); }
};

namespace {

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

// (sp_mix_row_ell below is a second copy of this kernel's sums, tree, factorisation and ell, and promises this kernel's bits: change both;
// tests/test_gpu_sparse_mix.py holds every K to it)
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

// ---- the mixture's row pass
struct SpMixRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const int32_t *rows;  // the bin's rows, local to the block
    int64_t nrows, row0;
    int W, d, nc;                    // nc <= MIX_MAX components of ONE state size
    const double *model[MIX_MAX];
    double *llk[MIX_MAX];            // component c's ell, indexed by global row (its row of the component-major buffer)
};

// ell of one row on its group of W lanes, sparse_row_kernel's statements in sparse_row_kernel's order: each(f) calls f(column, value)
// for this lane's entries of the row in order; the lane gathers the rows of C and accumulates its own [G | b | |x~|^2], one butterfly
// of log2 W steps adds the group's lanes, then every lane factors M = sigma^2 I + G and solves.  (A second copy of those statements,
// not a helper that both kernels call: moving sparse_row_kernel's into a function changed its registers and schedule.)
template <int K, class Each>
__device__ __forceinline__ double sp_mix_row_ell(Each each, int W, int m, const double *C, const double *mu, double s2, double lnsig) {
    constexpr int KP = K * (K + 1) / 2;
    double G[KP], b[K], xx = 0.0;
#pragma unroll
    for (int e = 0; e < KP; ++e) G[e] = 0.0;
#pragma unroll
    for (int t = 0; t < K; ++t) b[t] = 0.0;
    each([&](int j, double x) {
        const double xt = x - mu[j];
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
    });
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
    Posterior<K> post;
    double pm;
    int pe;
    post.factor([&](int e) { return G[e]; }, s2, pm, pe);
    double z[K], quad, zz;
    post.solve([&](int t) { return b[t]; }, z, quad, zz);
    // sample_llk(xx, quad, logdet, s2, lnsig, m, K), with the operations that sparse_row_kernel's compilation of it has written out.
    // Left to the compiler they differ here in two places: |x~|^2 - y^2 becomes one fused operation at K = 1, where quad is a bare
    // product with no other reader, and ln(2 pi) m, which does not depend on the component, is hoisted out of the component loop and
    // then added, not fused.  So: no contraction in this block, and the two multiply-adds of the row kernel as fma.
    const double logdet = Posterior<K>::logdet(pm, pe);
    if (m == 0) return 0.0;
    {
#pragma clang fp contract(off)
        const double resid = xx - quad;
        return -0.5 * fma(LN_2PI, (double)m, fma(2.0 * lnsig, (double)(m - K), resid / s2 + logdet));
    }
}

// sparse_row_kernel's lanes, rows and sums (sp_mix_row_ell) for a list of components: the row's list slot, row_ptr and -- REG, the two
// short bins, where a lane has at most 4 entries -- its (column, value) entries are fetched once and stay in registers across the
// component loop; without REG (the long bin; K >= 12, where the single-model kernel already holds one wave per SIMD) each component
// reads them again, from L1 / L2.  The component loop is rolled: the registers are the single-model kernel's plus the entries.
template <int K, bool REG>
__global__ __launch_bounds__(256) void sparse_mix_row_kernel(SpMixRowArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        const int m = (int)(e1 - e0);
        int jr[4] = {0, 0, 0, 0};
        double xr[4] = {0.0, 0.0, 0.0, 0.0};
        int cnt = 0;
        if (REG) {  // entries sub, sub + W, sub + 2 W, sub + 3 W: m <= 4 W in these bins
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t e = e0 + sub + (int64_t)i * W;
                if (e < e1) {
                    jr[i] = a.col[e];
                    xr[i] = a.val[e];
                    cnt = i + 1;
                }
            }
        }
#pragma unroll 1
        for (int c = 0; c < a.nc; ++c) {  // (uniform)
            const double *model = a.model[c];
            const double s2 = model[1], lnsig = model[2];
            const double *C = model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
            const double ell = sp_mix_row_ell<K>(
                [&](auto &&f) {
                    if (REG) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < cnt) f(jr[i], xr[i]);
                    } else {
                        for (int64_t e = e0 + sub; e < e1; e += W) f(a.col[e], a.val[e]);
                    }
                },
                W, m, C, mu, s2, lnsig);
            if (live && sub == 0) a.llk[c][r] = ell;
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

// the row r of [row0, row0 + rows) with qptr[r] <= e < qptr[r + 1]
__device__ __forceinline__ int64_t query_row(const int64_t *qptr, int64_t e, int64_t row0, int64_t rows) {
    int64_t lo = row0, hi = row0 + rows;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (qptr[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
// mean_j + c_j . z and c_j^T S c_j + sigma^2 of a new reading of column j in a row whose posterior is (z, S)
__device__ __forceinline__ void predict_entry(const double *model, int d, int k, int j, const double *z, const double *S, double &mean,
                                              double &var) {
    const double *C = model + MODEL_HDR, *mu = C + (int64_t)d * k;
    const double *c = C + (int64_t)j * k;
    double dot = 0.0, q = 0.0;
    for (int t = 0; t < k; ++t) {
        dot = fma(c[t], z[t], dot);
        double sc = 0.0;
        for (int u = 0; u < k; ++u) sc = fma(S[t * k + u], c[u], sc);
        q = fma(c[t], sc, q);
    }
    mean = mu[j] + dot;
    var = q + model[1];
}

// query entries [q0, q1) (the query rows of one block): mean_j + c_j . z_i, c_j^T Sigma_i c_j + sigma^2
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

// The mixture's predictive (ppca_mix_sparse_predict), component c of nm over the query entries [q0, q1) of one block: with r = the
// row's posterior weight of the component and (m, v) predict_entry's pair under it, cmean[c][e - q0] = m, mean[e] (+)= r m and
// var[e] (+)= r v (c = 0 assigns).  The thread that owns entry e adds the components in launch order = index order.
__global__ __launch_bounds__(256) void sparse_mix_predict_kernel(const int64_t *qptr, const int32_t *qcol, int64_t q0, int64_t q1, int64_t row0,
                                                                 int64_t rows, int d, int k, const double *model, const double *states,
                                                                 const double *covs, const double *logpost, int c, int nm, double *cmean,
                                                                 double *mean, double *var) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < q1; e += stride) {
        const int64_t row = query_row(qptr, e, row0, rows), lr = row - row0;
        double m, v;
        predict_entry(model, d, k, qcol[e], states + lr * k, covs + lr * k * k, m, v);
        const double r = exp(logpost[row * nm + c]);
        cmean[(int64_t)c * (q1 - q0) + (e - q0)] = m;
        mean[e] = c == 0 ? r * m : fma(r, m, mean[e]);
        var[e] = c == 0 ? r * v : fma(r, v, var[e]);
    }
}
// ... then the spread of the components' means around the mixture's: var[e] += sum_c r_c (m_c - mean[e])^2, in index order (a sum of
// squares, never a difference of them)
__global__ __launch_bounds__(256) void sparse_mix_spread_kernel(const int64_t *qptr, int64_t q0, int64_t q1, int64_t row0, int64_t rows,
                                                                const double *logpost, int nm, const double *cmean, const double *mean,
                                                                double *var) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = q0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < q1; e += stride) {
        const int64_t row = query_row(qptr, e, row0, rows);
        const double mu = mean[e];
        double s = 0.0;
        for (int c = 0; c < nm; ++c) {
            const double dv = cmean[(int64_t)c * (q1 - q0) + (e - q0)] - mu;
            s = fma(exp(logpost[row * nm + c]), dv * dv, s);
        }
        var[e] += s;
    }
}

// ---- held-out scoring
// One held entry x of column j (cj = c_j, muj = mean_j) in a row whose posterior given `train` is (z, S): e^2, v and l of the new
// reading.  m and v are sparse_predict_kernel's, multiply-add for multiply-add; l is heldout_score_kernel's expression.
template <int K>
__device__ __forceinline__ void held_entry(const double *cj, const double *z, const double *S, double x, double muj, double s2, double &e2,
                                           double &v, double &l) {
    double c[K];
#pragma unroll
    for (int t = 0; t < K; ++t) c[t] = cj[t];
    double dot = 0.0, q = 0.0;
    // One row of S at a time, the rows in a rolled loop: unrolled, the compiler keeps all K^2 elements of a row's S in registers across
    // the entries of sparse_held_row_kernel (512 VGPRs and spills from K = 15 on).
#pragma unroll 1
    for (int t = 0; t < K; ++t) {
        const double ct = cj[t];
        dot = fma(ct, z[t], dot);
        double sc = 0.0;
#pragma unroll
        for (int u = 0; u < K; ++u) sc = fma(S[t * K + u], c[u], sc);
        q = fma(ct, sc, q);
    }
    const double e = x - (muj + dot);
    e2 = __dmul_rn(e, e);
    v = q + s2;
    l = -0.5 * (LOG_2PI + log(v) + e2 / v);
}

struct SpHeldRowArgs {
    const int64_t *row_ptr;  // held's CSR
    const int32_t *col;
    const double *val;
    const int32_t *rows;  // a bin of held's rows, local to the block
    int64_t nrows, row0;
    int W, d;
    const double *model;
    const double *states, *covs;  // of train's rows, indexed by the row within the block
    double *per_row;              // indexed by global row
};

template <int K>
__global__ __launch_bounds__(256) void sparse_held_row_kernel(SpHeldRowArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1];
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        const double *z = a.states + lr * K, *S = a.covs + lr * (K * K);
        double lsum = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            double e2, v, l;
            held_entry<K>(C + (int64_t)j * K, z, S, a.val[e], mu[j], s2, e2, v, l);
            lsum += l;
        }
        // the group's lanes, one butterfly: the same tree for every row of the bin
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
            if (o < W) lsum += __shfl_xor(lsum, o, 64);
        if (live && sub == 0) a.per_row[r] = lsum;
    }
}

constexpr int SP_HELD_GW = 16;  // lanes of an item's group in sparse_held_col_kernel
constexpr int SP_HELD_NO = 4;   // sums per column: w | w l | w e^2 | w e^2 / v

struct SpHeldColArgs {
    const SpItem *items;  // held's work items, inverted index
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *w;  // train's weights (nullable), indexed by global row
    int64_t row0;
    const double *states, *covs;  // of train's rows, indexed by the row within the block
    const double *model;
    int d;
    double *colsum;  // 4 x d
    double *runpart;
};

template <int K>
__global__ __launch_bounds__(256) void sparse_held_col_kernel(SpHeldColArgs a) {
    constexpr int GW = SP_HELD_GW, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const double s2 = a.model[1];
    const double *C = a.model + MODEL_HDR, *mu = C + (int64_t)a.d * K;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double *cj = C + (int64_t)it.col * K;
        const double muj = mu[it.col];
        double acc[SP_HELD_NO] = {0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group) one chunk of GW entries, ascending row
            double p[SP_HELD_NO] = {0.0, 0.0, 0.0, 0.0};  // (past the end: exact zeros, which change no sum)
            if (t + sub < it.len) {
                const int64_t li = a.trow[it.start + t + sub];
                const double w = a.w ? a.w[a.row0 + li] : 1.0;
                double e2, v, l;
                held_entry<K>(cj, a.states + li * K, a.covs + li * (K * K), a.tval[it.start + t + sub], muj, s2, e2, v, l);
                p[0] = w;
                p[1] = w * l;
                p[2] = w * e2;
                p[3] = w * (e2 / v);
            }
#pragma unroll
            for (int o = 1; o < GW; o <<= 1)
#pragma unroll
                for (int q = 0; q < SP_HELD_NO; ++q) p[q] += __shfl_xor(p[q], o, 64);
#pragma unroll
            for (int q = 0; q < SP_HELD_NO; ++q) acc[q] += p[q];
        }
        if (live && sub < SP_HELD_NO) {
            const double s = sub == 0 ? acc[0] : sub == 1 ? acc[1] : sub == 2 ? acc[2] : acc[3];
            if (it.dest < 0)
                a.colsum[(int64_t)sub * a.d + it.col] += s;
            else
                a.runpart[it.dest * SP_HELD_NO + sub] = s;
        }
    }
}

// column sums of a long column += its runs' partials, added in run order: one thread per (column, sum)
__global__ __launch_bounds__(256) void sparse_held_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, double *colsum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_long * SP_HELD_NO; t += stride) {
        const SpLong lc = longs[t / SP_HELD_NO];
        const int q = (int)(t % SP_HELD_NO);
        double s = 0.0;
        for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * SP_HELD_NO + q];
        colsum[(int64_t)q * d + lc.col] += s;
    }
}

// ---- the column rescaling behind factor analysis on row-compressed data
struct SpScaleRowArgs {
    const int64_t *row_ptr;
    const int32_t *col;
    const double *val;
    const int32_t *rows;  // a bin of the block's rows, local to the block
    int64_t nrows, row0;
    int W;
    const double *a, *l;  // per column (l read only with rowsum)
    double *out_val;      // nullable, CSR order
    double *rowsum;       // nullable, indexed by global row
};

// The CSR orientation: the groups and bins of sparse_held_row_kernel.  Lane s of a row's group takes the entries s, s + W, ...: each
// gets out_val = val * a[col] (one fp64 multiply) and the lane adds l[col] in that order; one butterfly adds the lanes.  The gather of
// a[col] / l[col] is per entry (the columns of a row are scattered): 8 d bytes each, which stay in L2.
__global__ __launch_bounds__(256) void sparse_scale_row_kernel(SpScaleRowArgs a) {
    const int lane = threadIdx.x & 63, W = a.W, sub = lane & (W - 1), gpw = 64 / W;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * gpw; base < a.nrows; base += nwaves * gpw) {  // (uniform over the wave)
        const int64_t slot = base + lane / W;
        const bool live = slot < a.nrows;
        const int64_t lr = live ? a.rows[slot] : 0, r = a.row0 + lr;
        const int64_t e0 = live ? a.row_ptr[r] : 0, e1 = live ? a.row_ptr[r + 1] : 0;
        double lsum = 0.0;
        for (int64_t e = e0 + sub; e < e1; e += W) {
            const int j = a.col[e];
            if (a.out_val) a.out_val[e] = __dmul_rn(a.val[e], a.a[j]);
            if (a.rowsum) lsum += a.l[j];
        }
        if (a.rowsum) {  // (uniform) the group's lanes, one butterfly: the same tree for every row of the bin
#pragma unroll
            for (int o = 1; o < 64; o <<= 1)
                if (o < W) lsum += __shfl_xor(lsum, o, 64);
            if (live && sub == 0) a.rowsum[r] = lsum;
        }
    }
}

constexpr int SP_SCALE_GW = 16;  // lanes of an item's group in sparse_scale_col_kernel
constexpr int SP_SCALE_NO = 3;   // sums per column: w | w (x a - b) | w (x a - b)^2

struct SpScaleColArgs {
    const SpItem *items;  // the work items of the inverted index
    int64_t n_items;
    const int32_t *trow;
    const double *tval;
    const double *w;  // row weights (nullable), indexed by global row
    int64_t row0;
    const double *a, *b;  // per column
    int d;
    double *out_tval;  // nullable, inverted-index order
    double *colsum;    // nullable, 3 x d
    double *runpart;
};

// The index orientation: the work items, 16-lane groups and run partials of sparse_held_col_kernel.  Lane s takes the entries s,
// s + 16, ... of the item (ascending row): out_tval = tval * a_j, the multiply of the row kernel on the same operands, and
// [w | w r | w r^2] with r = x a_j - b_j.  Each chunk of 16 entries is added by one butterfly and the chunks in order.  A whole column
// adds into the 3 x d sums (blocks in stream order); a run writes a partial and sparse_scale_fix_kernel adds a column's runs in run
// order.  a_j and b_j are uniform over the group.  No float atomics.
__global__ __launch_bounds__(256) void sparse_scale_col_kernel(SpScaleColArgs a) {
    constexpr int GW = SP_SCALE_GW, GPW = 64 / GW;
    const int lane = threadIdx.x & 63, sub = lane & (GW - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * GPW; base < a.n_items; base += nwaves * GPW) {  // (uniform over the wave)
        const int64_t ii = base + lane / GW;
        const bool live = ii < a.n_items;
        const SpItem it = live ? a.items[ii] : SpItem{0, -1, 0, 0};
        const double aj = a.a[it.col], bj = a.b[it.col];
        double acc[SP_SCALE_NO] = {0.0, 0.0, 0.0};
        for (int t = 0; t < it.len; t += GW) {  // (uniform over the group) one chunk of GW entries, ascending row
            double p[SP_SCALE_NO] = {0.0, 0.0, 0.0};  // (past the end: exact zeros, which change no sum)
            if (t + sub < it.len) {
                const int64_t at = it.start + t + sub;
                const double y = __dmul_rn(a.tval[at], aj);
                if (a.out_tval) a.out_tval[at] = y;
                if (a.colsum) {
                    const double w = a.w ? a.w[a.row0 + a.trow[at]] : 1.0;
                    const double r = y - bj;
                    p[0] = w;
                    p[1] = w * r;
                    p[2] = w * __dmul_rn(r, r);
                }
            }
            if (a.colsum) {  // (uniform)
#pragma unroll
                for (int o = 1; o < GW; o <<= 1)
#pragma unroll
                    for (int q = 0; q < SP_SCALE_NO; ++q) p[q] += __shfl_xor(p[q], o, 64);
#pragma unroll
                for (int q = 0; q < SP_SCALE_NO; ++q) acc[q] += p[q];
            }
        }
        if (a.colsum && live && sub < SP_SCALE_NO) {
            const double s = sub == 0 ? acc[0] : sub == 1 ? acc[1] : acc[2];
            if (it.dest < 0)
                a.colsum[(int64_t)sub * a.d + it.col] += s;
            else
                a.runpart[it.dest * SP_SCALE_NO + sub] = s;
        }
    }
}

// column sums of a long column += its runs' partials, added in run order: one thread per (column, sum)
__global__ __launch_bounds__(256) void sparse_scale_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, double *colsum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_long * SP_SCALE_NO; t += stride) {
        const SpLong lc = longs[t / SP_SCALE_NO];
        const int q = (int)(t % SP_SCALE_NO);
        double s = 0.0;
        for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * SP_SCALE_NO + q];
        colsum[(int64_t)q * d + lc.col] += s;
    }
}

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


#define SP_DISPATCH(k, F, ...)                  \
    switch (k) {                                \
        case 1: return F<1>(__VA_ARGS__);       \
        case 2: return F<2>(__VA_ARGS__);       \
        case 3: return F<3>(__VA_ARGS__);       \
        case 4: return F<4>(__VA_ARGS__);       \
        case 5: return F<5>(__VA_ARGS__);       \
        case 6: return F<6>(__VA_ARGS__);       \
        case 7: return F<7>(__VA_ARGS__);       \
        case 8: return F<8>(__VA_ARGS__);       \
        case 9: return F<9>(__VA_ARGS__);       \
        case 10: return F<10>(__VA_ARGS__);     \
        case 11: return F<11>(__VA_ARGS__);     \
        case 12: return F<12>(__VA_ARGS__);     \
        case 13: return F<13>(__VA_ARGS__);     \
        case 14: return F<14>(__VA_ARGS__);     \
        case 15: return F<15>(__VA_ARGS__);     \
        case 16: return F<16>(__VA_ARGS__);     \
        default: return hipErrorInvalidValue;   \
    }

template <int K>
hipError_t row_t(const SpRowArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((sparse_row_kernel<K>), dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <int K>
hipError_t col_t(const SpColArgs &a, int n_cu, hipStream_t s) {
    constexpr int per_wg = 4 * (64 / SpColCfg<K>::GW);
    const int64_t want = (a.n_items + per_wg - 1) / per_wg;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)std::max(n_cu, 1) * 8));
    hipLaunchKernelGGL((sparse_col_kernel<K>), dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <int K>
hipError_t held_row_t(const SpHeldRowArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((sparse_held_row_kernel<K>), dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <int K>
hipError_t held_col_t(const SpHeldColArgs &a, int n_cu, hipStream_t s) {
    constexpr int per_wg = 4 * (64 / SP_HELD_GW);
    const int64_t want = (a.n_items + per_wg - 1) / per_wg;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)std::max(n_cu, 1) * 8));
    hipLaunchKernelGGL((sparse_held_col_kernel<K>), dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_held_row(int k, const SpHeldRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, held_row_t, a, grid, s); }
hipError_t launch_held_col(int k, const SpHeldColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, held_col_t, a, n_cu, s); }
hipError_t launch_row(int k, const SpRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, row_t, a, grid, s); }
hipError_t launch_col(int k, const SpColArgs &a, int n_cu, hipStream_t s) { SP_DISPATCH(k, col_t, a, n_cu, s); }
template <int K>
hipError_t mix_row_t(const SpMixRowArgs &a, int grid, hipStream_t s) {
    if constexpr (K < 12) {  // a lane's entries in registers: a bin where it has at most 4 of them, and a register budget with room for them
        if (a.W < 64) {
            hipLaunchKernelGGL((sparse_mix_row_kernel<K, true>), dim3((unsigned)grid), dim3(256), 0, s, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((sparse_mix_row_kernel<K, false>), dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_mix_row(int k, const SpMixRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, mix_row_t, a, grid, s); }
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
    const int64_t items = sp_top_tiles(g.rows, var) * g.nchunks;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + 3) / 4, (int64_t)std::max(n_cu, 1) * 8));
    if (var)
        hipLaunchKernelGGL((sparse_topn_kernel<K, true, SP_TOP_RV>), dim3((unsigned)grid), dim3(256), 0, s, p.row_ptr, p.col, p.cand, p.model,
                           p.states, p.covs, p.ps, p.pc, g);
    else
        hipLaunchKernelGGL((sparse_topn_kernel<K, false, SP_TOP_R>), dim3((unsigned)grid), dim3(256), 0, s, p.row_ptr, p.col, p.cand, p.model,
                           p.states, p.covs, p.ps, p.pc, g);
    return hipGetLastError();
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
    const int64_t items = sp_top_tiles(g.rows, var) * g.nchunks;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + 3) / 4, (int64_t)std::max(n_cu, 1) * 8));
    if (var)
        hipLaunchKernelGGL((sparse_mix_topn_kernel<K, true, SP_TOP_RV>), dim3((unsigned)grid), dim3(256), 0, s, p.row_ptr, p.col, p.cand,
                           p.comps, p.resp, p.states, p.covs, p.ps, p.pc, g, p.nm, p.cap, -(double)INFINITY);
    else
        hipLaunchKernelGGL((sparse_mix_topn_kernel<K, false, SP_TOP_R>), dim3((unsigned)grid), dim3(256), 0, s, p.row_ptr, p.col, p.cand,
                           p.comps, p.resp, p.states, p.covs, p.ps, p.pc, g, p.nm, p.cap, -(double)INFINITY);
    return hipGetLastError();
}
hipError_t launch_mix_topn(int k, const SpMixTopPtrs &p, const SpTopDims &g, bool var, int n_cu, hipStream_t s) {
    SP_DISPATCH(k, mix_topn_t, p, g, var, n_cu, s);
}
// one of the two element-wise helpers of the mixture's top-n, over len outputs
int sp_elementwise_grid(int64_t len, int n_cu) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((len + 255) / 256, (int64_t)std::max(n_cu, 1) * 16));
}

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

int sp_upload(ppca_ctx *ctx, const void *src, size_t bytes, BufRef *out) {
    if (int rc = dev_alloc(std::max<size_t>(bytes, 8), out)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync((*out)->p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PPCA_OK;
}

int sp_check(const ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model) {
    if (!ctx || !sp || !model) return fail(PPCA_ERR_INVALID, "null argument");
    if (sp->core->d != model->d)
        return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", sp->core->d, model->d);
    if (sp->ctx->device != model->ctx->device) return fail(PPCA_ERR_INVALID, "dataset and model live on different devices");
    if (model->k > SP_MAX_K)
        return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported on sparse data: the kernels cover k <= %d", model->k, SP_MAX_K);
    if (sp->core->n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    return PPCA_OK;
}

int sp_row_grid(int64_t nrows, int W, int n_cu) {
    const int per_wg = 4 * (64 / W);
    return (int)std::max<int64_t>(1, std::min<int64_t>((nrows + per_wg - 1) / per_wg, (int64_t)std::max(n_cu, 1) * 8));
}

// the row pass over one block: outputs indexed by the row within the block
int sp_rows_of_block(ppca_ctx *ctx, const ppca_sparse *sp, const SpBlock &b, const ppca_model *model, double *llks, double *states, double *covs,
                     double *rec, double *rscal) {
    const SpCore &c = *sp->core;
    static const int widths[3] = {4, 16, 64};
    for (int bin = 0; bin < 3; ++bin) {
        if (b.nbin[bin] == 0) continue;
        SpRowArgs a{};
        a.row_ptr = static_cast<const int64_t *>(c.row_ptr->p);
        a.col = static_cast<const int32_t *>(c.col->p);
        a.val = sp->val();
        a.w = sp->w;
        a.rows = static_cast<const int32_t *>(b.rowlist->p) + b.bin_off[bin];
        a.nrows = b.nbin[bin];
        a.row0 = b.row0;
        a.W = widths[bin];
        a.d = c.d;
        a.model = model->p();
        a.llks = llks;
        a.states = states;
        a.covs = covs;
        a.rec = rec;
        a.rscal = rscal;
        HIP_TRY(launch_row(model->k, a, sp_row_grid(a.nrows, a.W, ctx->n_cu), ctx->stream));
    }
    return PPCA_OK;
}

// scal8 (+)= the block's eight scalars; spart: ceil(max_rows / 1024) x 8 doubles of scratch
int sp_block_scalars(ppca_ctx *ctx, const SpBlock &b, const double *rscal, double *spart, double *scal8, int accumulate) {
    const int parts = (int)((b.rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS);
    hipLaunchKernelGGL(sparse_scal_kernel, dim3((unsigned)parts), dim3(256), 0, ctx->stream, rscal, b.rows, spart);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_reduce_partials(spart, parts, 8, scal8, ctx->stream, accumulate));
    return PPCA_OK;
}

// the scratch of sp_accumulate at state size k: one block's records and scalar terms, the scalars' partials, the runs' partials
struct SpAccScratch {
    BufRef rec, rscal, spart, runpart;
};
int sp_acc_scratch(const SpCore &c, int k, SpAccScratch *s) {
    const int nr = k + 1 + k * (k + 1) / 2;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * nr, &s->rec)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * SP_NSCAL, &s->rscal)) return rc;
    if (int rc = dev_alloc(sizeof(double) * 8 * (size_t)((c.max_rows + SP_SCAL_ROWS - 1) / SP_SCAL_ROWS), &s->spart)) return rc;
    return dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * sp_no(k), &s->runpart);
}

// scratch: nullptr = taken here; the mixture step hands in ONE, sized for its largest state size, taken before its first launch
int sp_accumulate(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, double *stats, const SpAccScratch *scratch = nullptr) {
    const SpCore &c = *sp->core;
    const int k = model->k;
    const StatsLayout L(c.d, k);
    SpAccScratch own;
    if (!scratch) {
        if (int rc = sp_acc_scratch(c, k, &own)) return rc;
        scratch = &own;
    }
    const BufRef &rec = scratch->rec, &rscal = scratch->rscal, &spart = scratch->spart, &runpart = scratch->runpart;
    HIP_TRY(hipMemsetAsync(stats, 0, sizeof(double) * (size_t)L.len, ctx->stream));
    for (size_t bi = 0; bi < c.blocks.size(); ++bi) {
        const SpBlock &b = c.blocks[bi];
        double *recp = static_cast<double *>(rec->p), *rs = static_cast<double *>(rscal->p);
        if (int rc = sp_rows_of_block(ctx, sp, b, model, nullptr, nullptr, nullptr, recp, rs)) return rc;
        if (int rc = sp_block_scalars(ctx, b, rs, static_cast<double *>(spart->p), stats + L.scalars, 1)) return rc;
        if (b.n_items == 0) continue;
        SpColArgs a{};
        a.items = static_cast<const SpItem *>(b.items->p);
        a.n_items = b.n_items;
        a.trow = static_cast<const int32_t *>(c.trow->p);
        a.tval = sp->tval();
        a.rec = recp;
        a.model = model->p();
        a.d = c.d;
        a.stats = stats;
        a.runpart = static_cast<double *>(runpart->p);
        HIP_TRY(launch_col(k, a, ctx->n_cu, ctx->stream));
        if (b.n_long > 0) {
            const int grid = (int)std::min<int64_t>(b.n_long, (int64_t)std::max(ctx->n_cu, 1) * 8);
            hipLaunchKernelGGL(sparse_fix_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, static_cast<const SpLong *>(b.longs->p),
                               b.n_long, static_cast<const double *>(runpart->p), c.d, k, stats);
            HIP_TRY(hipGetLastError());
        }
    }
    return PPCA_OK;
}

}  // namespace

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
        if ((rc = sp_upload(ctx, row_ptr, sizeof(int64_t) * (size_t)(n + 1), &core->row_ptr))) break;
        if ((rc = sp_upload(ctx, col, sizeof(int32_t) * (size_t)nnz, &core->col))) break;
        if ((rc = sp_upload(ctx, val, sizeof(double) * (size_t)nnz, &core->val))) break;
        if ((rc = sp_upload(ctx, trow.data(), sizeof(int32_t) * (size_t)nnz, &core->trow))) break;
        if ((rc = sp_upload(ctx, tval.data(), sizeof(double) * (size_t)nnz, &core->tval))) break;
        for (size_t i = 0; i < hb.size() && !rc; ++i) {
            SpBlock &b = core->blocks[i];
            if ((rc = sp_upload(ctx, hb[i].rows.data(), sizeof(int32_t) * hb[i].rows.size(), &b.rowlist))) break;
            if ((rc = sp_upload(ctx, hb[i].items.data(), sizeof(SpItem) * hb[i].items.size(), &b.items))) break;
            if ((rc = sp_upload(ctx, hb[i].longs.data(), sizeof(SpLong) * hb[i].longs.size(), &b.longs))) break;
        }
        if (rc) break;
        if (weights) {
            if ((rc = sp_upload(ctx, weights, sizeof(double) * (size_t)n, &sp->wbuf))) break;
            sp->w = static_cast<const double *>(sp->wbuf->p);
        }
    } while (false);
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // the uploads read this call's host buffers
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
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
        nd->w = static_cast<const double *>(nd->wbuf->p);
    }
    *out = nd.release();
    return PPCA_OK;
}

extern "C" int ppca_sparse_to_host(ppca_sparse *sp, int64_t *row_ptr, int32_t *col, double *val, double *weights) {
    if (!sp) return fail(PPCA_ERR_INVALID, "null argument");
    ppca_ctx *ctx = sp->ctx;
    USE_CTX(ctx);
    const SpCore &c = *sp->core;
    if (row_ptr) HIP_TRY(hipMemcpyAsync(row_ptr, c.row_ptr->p, sizeof(int64_t) * (size_t)(c.n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (col && c.nnz) HIP_TRY(hipMemcpyAsync(col, c.col->p, sizeof(int32_t) * (size_t)c.nnz, hipMemcpyDeviceToHost, ctx->stream));
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
    double *stats = static_cast<double *>(ctx->stats->p);
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
    double *stats = static_cast<double *>(ctx->stats->p);
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
    for (const SpBlock &b : c.blocks) {
        if (int rc = sp_rows_of_block(ctx, sp, b, model, static_cast<double *>(llks->p) + b.row0, nullptr, nullptr, nullptr,
                                      static_cast<double *>(rscal->p)))
            return rc;
        if (int rc = sp_block_scalars(ctx, b, static_cast<double *>(rscal->p), static_cast<double *>(spart->p), static_cast<double *>(scal->p), 1))
            return rc;
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
        if (int rc = sp_rows_of_block(ctx, sp, b, model, nullptr, static_cast<double *>(st->p), cv ? static_cast<double *>(cv->p) : nullptr,
                                      nullptr, nullptr))
            return rc;
        HIP_TRY(hipMemcpyAsync(states_host + b.row0 * k, st->p, sizeof(double) * (size_t)b.rows * k, hipMemcpyDeviceToHost, ctx->stream));
        if (covs_host)
            HIP_TRY(hipMemcpyAsync(covs_host + b.row0 * k * k, cv->p, sizeof(double) * (size_t)b.rows * k * k, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // the next block overwrites the scratch
    }
    return PPCA_OK;
}

// the query pattern of a predict call; *nq = its entries (0: nothing to do, the outputs may be null)
static int sp_check_query(const SpCore &c, const int64_t *query_row_ptr, const int32_t *query_col, const double *mean_host,
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

extern "C" int ppca_sparse_predict(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, const int64_t *query_row_ptr,
                                   const int32_t *query_col, double *mean_host, double *var_host) {
    if (int rc = sp_check(ctx, sp, model)) return rc;
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
        rc = sp_rows_of_block(ctx, sp, b, model, nullptr, static_cast<double *>(st->p), static_cast<double *>(cv->p), nullptr, nullptr);
        if (rc) break;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((q1 - q0 + 255) / 256, (int64_t)std::max(ctx->n_cu, 1) * 16));
        hipLaunchKernelGGL(sparse_predict_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, static_cast<const int64_t *>(qp->p),
                           static_cast<const int32_t *>(qc->p), q0, q1, b.row0, b.rows, c.d, k, model->p(), static_cast<const double *>(st->p),
                           static_cast<const double *>(cv->p), static_cast<double *>(mean->p), static_cast<double *>(var->p));
        if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "predict launch failed");
    }
    if (!rc && hipMemcpyAsync(mean_host, mean->p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(var_host, var->p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's buffers)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "predict failed: %s", hipGetErrorString(e));
    return PPCA_OK;
}

// ------------------------------------------------------------------ the mixture on row-compressed data
namespace {

int sp_mix_check(const ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t nm) {
    if (!ctx || !sp || !models || !log_weights) return fail(PPCA_ERR_INVALID, "null argument");
    if (nm < 1) return fail(PPCA_ERR_INVALID, "a mixture needs at least one component");
    for (int c = 0; c < nm; ++c) {
        if (!models[c]) return fail(PPCA_ERR_INVALID, "null model (component %d)", c);
        if (sp->core->d != models[c]->d)
            return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but component %d has output size %d", sp->core->d, c, models[c]->d);
        if (sp->ctx->device != models[c]->ctx->device) return fail(PPCA_ERR_INVALID, "dataset and component %d live on different devices", c);
    }
    for (int c = 0; c < nm; ++c)
        if (models[c]->k > SP_MAX_K)
            return fail(PPCA_ERR_UNSUPPORTED, "state size %d (component %d) is not supported on sparse data: the kernels cover k <= %d",
                        models[c]->k, c, SP_MAX_K);
    if (sp->core->n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    return PPCA_OK;
}

// llk[c n + i] = ell of row i under component c: the components grouped by state size, one launch of sparse_mix_row_kernel per group
// of at most MIX_MAX, block and non-empty bin
int sp_mix_rows(ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, int nm, double *llk) {
    const SpCore &c = *sp->core;
    static const int widths[3] = {4, 16, 64};
    std::vector<char> done((size_t)nm, 0);
    for (int first = 0; first < nm; ++first) {
        if (done[first]) continue;
        const int k = models[first]->k;
        std::vector<int> group;
        for (int e = first; e < nm; ++e)
            if (!done[e] && models[e]->k == k) {
                group.push_back(e);
                done[e] = 1;
            }
        for (size_t g0 = 0; g0 < group.size(); g0 += MIX_MAX) {
            SpMixRowArgs a{};
            a.row_ptr = static_cast<const int64_t *>(c.row_ptr->p);
            a.col = static_cast<const int32_t *>(c.col->p);
            a.val = sp->val();
            a.d = c.d;
            a.nc = (int)std::min<size_t>(MIX_MAX, group.size() - g0);
            for (int i = 0; i < a.nc; ++i) {
                a.model[i] = models[group[g0 + i]]->p();
                a.llk[i] = llk + (size_t)group[g0 + i] * c.n;
            }
            for (const SpBlock &b : c.blocks)
                for (int bin = 0; bin < 3; ++bin) {
                    if (b.nbin[bin] == 0) continue;
                    a.rows = static_cast<const int32_t *>(b.rowlist->p) + b.bin_off[bin];
                    a.nrows = b.nbin[bin];
                    a.row0 = b.row0;
                    a.W = widths[bin];
                    HIP_TRY(launch_mix_row(k, a, sp_row_grid(a.nrows, a.W, ctx->n_cu), ctx->stream));
                }
        }
    }
    return PPCA_OK;
}

struct SpMixDev {
    double *llk, *u, *lse, *logpost;
    MixAux ax;
};
// every block the posteriors need, in the context's mixture scratch (kept across iterations)
int sp_mix_blocks(ppca_ctx *ctx, int64_t n, int nm, bool want_logpost, SpMixDev *m) {
    if (int rc = ensure(ctx->mix[0], ctx->mix_cap[0], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = ensure(ctx->mix[1], ctx->mix_cap[1], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = ensure(ctx->mix[2], ctx->mix_cap[2], sizeof(double) * (size_t)n)) return rc;
    if (want_logpost)
        if (int rc = ensure(ctx->mix[3], ctx->mix_cap[3], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = mix_aux(ctx, nm, m->ax)) return rc;
    if (int rc = ensure_hstage(ctx, sizeof(double) * m->ax.P + sizeof(int) * (size_t)nm)) return rc;
    m->llk = static_cast<double *>(ctx->mix[0]->p);
    m->u = static_cast<double *>(ctx->mix[1]->p);
    m->lse = static_cast<double *>(ctx->mix[2]->p);
    m->logpost = want_logpost ? static_cast<double *>(ctx->mix[3]->p) : nullptr;
    return PPCA_OK;
}
// ell of every component, then u = ln w + log posterior, the rows' mixture log-density and (nullable) the log posteriors
int sp_mix_posteriors(ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int nm, const SpMixDev &m) {
    if (int rc = sp_mix_rows(ctx, sp, models, nm, m.llk)) return rc;
    if (int rc = mix_upload_logw(ctx, log_weights, nm, m.ax)) return rc;
    HIP_TRY(launch_mix_posteriors(m.llk, m.ax.logw, sp->w, sp->core->n, nm, m.u, m.lse, m.logpost, ctx->stream));
    return PPCA_OK;
}

}  // namespace

extern "C" int ppca_mix_sparse_component_llks(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, int32_t n_models, double *out_host) {
    static const double none = 0.0;  // (no weights are read)
    if (!out_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_mix_check(ctx, sp, models, &none, n_models)) return rc;
    USE_CTX(ctx);
    const size_t len = (size_t)n_models * sp->core->n;
    if (int rc = ensure(ctx->mix[0], ctx->mix_cap[0], sizeof(double) * len)) return rc;
    if (int rc = sp_mix_rows(ctx, sp, models, n_models, static_cast<double *>(ctx->mix[0]->p))) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, ctx->mix[0]->p, sizeof(double) * len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PPCA_OK;
}

extern "C" int ppca_mix_sparse_llk(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                                   double *total_host, double *per_row_host, double *log_posteriors_host) {
    if (int rc = sp_mix_check(ctx, sp, models, log_weights, n_models)) return rc;
    USE_CTX(ctx);
    const int64_t n = sp->core->n;
    SpMixDev m;
    if (int rc = sp_mix_blocks(ctx, n, n_models, log_posteriors_host != nullptr, &m)) return rc;
    if (int rc = sp_mix_posteriors(ctx, sp, models, log_weights, n_models, m)) return rc;
    double *work = static_cast<double *>(ctx->work->p);
    HIP_TRY(launch_reduce_sum(m.lse, sp->w, n, work + 1024, work, ctx->stream));
    double *hs = static_cast<double *>(ctx->hstage);  // (the context's staging buffer, not a local: an early return below leaves the copy pending)
    HIP_TRY(hipMemcpyAsync(hs, work + 1024, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (per_row_host) HIP_TRY(hipMemcpyAsync(per_row_host, m.lse, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (log_posteriors_host)
        HIP_TRY(hipMemcpyAsync(log_posteriors_host, m.logpost, sizeof(double) * (size_t)n * n_models, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (total_host) *total_host = hs[0];
    return PPCA_OK;
}

extern "C" int ppca_mix_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models_in, const double *log_weights_in,
                                       int32_t n_models, const ppca_prior *prior, ppca_model *const *models_out, double *log_weights_out,
                                       double *llk_in) {
    if (!models_out || !log_weights_out) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_mix_check(ctx, sp, models_in, log_weights_in, n_models)) return rc;
    const int nm = n_models;
    for (int c = 0; c < nm; ++c) {
        if (!models_out[c]) return fail(PPCA_ERR_INVALID, "null output model");
        if (models_out[c]->d != models_in[c]->d || models_out[c]->k != models_in[c]->k)
            return fail(PPCA_ERR_INVALID, "model shapes differ (component %d)", c);
        if (models_out[c] == models_in[c] || models_out[c]->buf == models_in[c]->buf)
            return fail(PPCA_ERR_INVALID, "out may not alias model_in (component %d)", c);
    }
    if (int rc = check_prior(prior)) return rc;
    USE_CTX(ctx);
    const SpCore &core = *sp->core;
    const int64_t n = core.n;
    // packed buffer: [statistics of component 0 | ... | nm weight sums | llk]; components may differ in state size
    std::vector<int64_t> off((size_t)nm + 1, 0);
    int kmax = 1;
    for (int c = 0; c < nm; ++c) {
        off[c + 1] = off[c] + StatsLayout(core.d, models_in[c]->k).len;
        kmax = std::max(kmax, models_in[c]->k);
    }
    const int64_t sums_at = off[nm], llk_at = sums_at + nm, total = llk_at + 1;
    // every device block of the step, before its first launch
    if (int rc = ensure(ctx->mixpack, ctx->mixpack_cap, sizeof(double) * (size_t)total)) return rc;
    SpMixDev m;
    if (int rc = sp_mix_blocks(ctx, n, nm, false, &m)) return rc;
    if (int rc = ensure(ctx->mix[4], ctx->mix_cap[4], sizeof(double) * (size_t)n)) return rc;
    SpAccScratch scratch;
    if (int rc = sp_acc_scratch(core, kmax, &scratch)) return rc;
    double *pack = static_cast<double *>(ctx->mixpack->p), *work = static_cast<double *>(ctx->work->p);
    double *aux = m.ax.shift, *wc = static_cast<double *>(ctx->mix[4]->p);
    if (int rc = sp_mix_posteriors(ctx, sp, models_in, log_weights_in, nm, m)) return rc;
    HIP_TRY(launch_reduce_sum(m.lse, sp->w, n, pack + llk_at, work, ctx->stream));
    for (int c = 0; c < nm; ++c) HIP_TRY(launch_reduce_max(m.u + (size_t)c * n, n, aux + c, work, ctx->stream));
    HIP_TRY(launch_mix_shift(aux, nm, ctx->stream));
    ctx->stats_llk_at = -1;
    ppca_sparse view;  // the same entries, row lists and index under the component's weights exp(u_c - shift_c)
    view.ctx = sp->ctx;
    view.core = sp->core;
    view.vbuf = sp->vbuf;
    view.tvbuf = sp->tvbuf;
    view.w = wc;
    for (int c = 0; c < nm; ++c) {
        HIP_TRY(launch_exp_shift(m.u + (size_t)c * n, aux + c, n, wc, ctx->stream));
        HIP_TRY(launch_reduce_sum(wc, nullptr, n, pack + sums_at + c, work, ctx->stream));
        if (int rc = sp_accumulate(ctx, &view, models_in[c], pack + off[c], &scratch)) return rc;
    }
    for (int c = 0; c < nm; ++c)
        if (int rc = em_finalize_plain(ctx, models_in[c], pack + off[c], prior, models_out[c])) return rc;
    HIP_TRY(launch_mix_logweights(pack + sums_at, aux, pack + llk_at, nm, m.ax.out, ctx->stream));
    double *hs = static_cast<double *>(ctx->hstage);
    HIP_TRY(hipMemcpyAsync(hs, m.ax.out, sizeof(double) * (size_t)(nm + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < nm; ++c) log_weights_out[c] = hs[c];
    if (llk_in) *llk_in = hs[nm];
    ctx->mix_rows_used.assign((size_t)nm, n);  // (no row is dropped here: the row lists and the index are fixed)
    return PPCA_OK;
}

extern "C" int ppca_mix_sparse_predict(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                                       const int64_t *query_row_ptr, const int32_t *query_col, double *mean_host, double *var_host) {
    if (int rc = sp_mix_check(ctx, sp, models, log_weights, n_models)) return rc;
    const SpCore &c = *sp->core;
    const int nm = n_models;
    int64_t nq = 0;
    if (int rc = sp_check_query(c, query_row_ptr, query_col, mean_host, var_host, &nq)) return rc;
    if (nq == 0) return PPCA_OK;
    USE_CTX(ctx);
    int kmax = 1;
    for (int e = 0; e < nm; ++e) kmax = std::max(kmax, models[e]->k);
    int64_t qmax = 0;  // the most query entries of a block
    for (const SpBlock &b : c.blocks) qmax = std::max(qmax, query_row_ptr[b.row0 + b.rows] - query_row_ptr[b.row0]);
    SpMixDev m;
    if (int rc = sp_mix_blocks(ctx, c.n, nm, true, &m)) return rc;
    BufRef st, cv, qp, qc, mean, var, cmean;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * kmax, &st)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * kmax * kmax, &cv)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &mean)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &var)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)qmax * nm, &cmean)) return rc;
    int rc = sp_upload(ctx, query_row_ptr, sizeof(int64_t) * (size_t)(c.n + 1), &qp);
    if (!rc) rc = sp_upload(ctx, query_col, sizeof(int32_t) * (size_t)nq, &qc);
    if (!rc) rc = sp_mix_posteriors(ctx, sp, models, log_weights, nm, m);
    const int64_t *qpd = qp ? static_cast<const int64_t *>(qp->p) : nullptr;
    const int32_t *qcd = qc ? static_cast<const int32_t *>(qc->p) : nullptr;
    double *stp = static_cast<double *>(st->p), *cvp = static_cast<double *>(cv->p), *cmp = static_cast<double *>(cmean->p);
    double *mp = static_cast<double *>(mean->p), *vp = static_cast<double *>(var->p);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        const int64_t q0 = query_row_ptr[b.row0], q1 = query_row_ptr[b.row0 + b.rows];
        if (q1 == q0) continue;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((q1 - q0 + 255) / 256, (int64_t)std::max(ctx->n_cu, 1) * 16));
        for (int e = 0; e < nm && !rc; ++e) {  // component by component: the scratch is ONE component's states and covariances
            rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, stp, cvp, nullptr, nullptr);
            if (rc) break;
            hipLaunchKernelGGL(sparse_mix_predict_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, qpd, qcd, q0, q1, b.row0, b.rows, c.d,
                               models[e]->k, models[e]->p(), stp, cvp, m.logpost, e, nm, cmp, mp, vp);
            if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "mixture predict launch failed");
        }
        if (rc) break;
        hipLaunchKernelGGL(sparse_mix_spread_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, qpd, q0, q1, b.row0, b.rows, m.logpost, nm,
                           cmp, mp, vp);
        if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "mixture predict launch failed");
    }
    if (!rc && hipMemcpyAsync(mean_host, mp, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(var_host, vp, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's buffers)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "mixture predict failed: %s", hipGetErrorString(e));
    return PPCA_OK;
}

// ------------------------------------------------------------------ top-n ranking (DESIGN.md sections 4.22 and 4.24)
namespace {

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
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((b.rows + 3) / 4, (int64_t)std::max(ctx->n_cu, 1) * 8));
        hipLaunchKernelGGL(sparse_topn_merge_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, static_cast<const double *>(o.ps->p),
                           static_cast<const int32_t *>(o.pc->p), b.rows, g.nchunks, n_top, static_cast<double *>(o.os->p),
                           static_cast<int32_t *>(o.oc->p));
        if (hipGetLastError() != hipSuccess) return fail(PPCA_ERR_HIP, "top-n merge launch failed");
    }
    if (hipMemcpyAsync(scores_host + b.row0 * n_top, o.os->p, sizeof(double) * (size_t)b.rows * n_top, hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipMemcpyAsync(cols_host + b.row0 * n_top, o.oc->p, sizeof(int32_t) * (size_t)b.rows * n_top, hipMemcpyDeviceToHost, ctx->stream) !=
            hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)  // (the next block overwrites the scratch)
        return fail(PPCA_ERR_HIP, "top-n failed: %s", hipGetErrorString(hipGetLastError()));
    return PPCA_OK;
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
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        rc = sp_rows_of_block(ctx, sp, b, model, nullptr, static_cast<double *>(st->p), var ? static_cast<double *>(cv->p) : nullptr, nullptr,
                              nullptr);
        if (rc) break;
        const SpTopDims g = sp_top_dims(ctx, c, b, n_top, kappa, exclude_observed, nc);
        SpTopPtrs p{};
        p.row_ptr = static_cast<const int64_t *>(c.row_ptr->p);
        p.col = static_cast<const int32_t *>(c.col->p);
        p.cand = candidates ? static_cast<const int32_t *>(cd->p) : nullptr;
        p.model = model->p();
        p.states = static_cast<const double *>(st->p);
        p.covs = var ? static_cast<const double *>(cv->p) : nullptr;
        p.ps = static_cast<double *>(g.final ? o.os->p : o.ps->p);
        p.pc = static_cast<int32_t *>(g.final ? o.oc->p : o.pc->p);
        if (launch_topn(k, p, g, var, ctx->n_cu, ctx->stream) != hipSuccess) {
            rc = fail(PPCA_ERR_HIP, "top-n launch failed");
            break;
        }
        rc = sp_top_finish(ctx, b, g, o, cols_host, scores_host);
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the upload reads the caller's buffer)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "top-n failed: %s", hipGetErrorString(e));
    return PPCA_OK;
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
            double *pd = static_cast<double *>(padded[e]->p);
            hipLaunchKernelGGL(sparse_pad_kernel, dim3((unsigned)sp_elementwise_grid((int64_t)c.d * K, ctx->n_cu)), dim3(256), 0, ctx->stream,
                               comps[e].C, (int64_t)c.d, ke, K, 0, pd);
            if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
            comps[e].C = pd;
        }
    }
    SpMixComp *table_dev = static_cast<SpMixComp *>(table->p);
    if (!rc && hipMemcpyAsync(table_dev, comps.data(), sizeof(SpMixComp) * (size_t)nm, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "upload failed");
    if (!rc && candidates) rc = sp_upload(ctx, candidates, sizeof(int32_t) * (size_t)n_candidates, &cd);
    if (!rc) rc = sp_mix_posteriors(ctx, sp, models, log_weights, nm, m);
    double *stp = static_cast<double *>(st->p), *cvp = var ? static_cast<double *>(cv->p) : nullptr, *rp = static_cast<double *>(resp->p);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        hipLaunchKernelGGL(sparse_mix_resp_kernel, dim3((unsigned)sp_elementwise_grid(b.rows * nm, ctx->n_cu)), dim3(256), 0, ctx->stream,
                           m.logpost + b.row0 * nm, b.rows * nm, rp);
        if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
        for (int e = 0; e < nm && !rc; ++e) {
            const int ke = models[e]->k;
            double *zs = stp + cap * e * K, *ss = var ? cvp + cap * e * K * K : nullptr;
            if (ke == K) {
                rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, zs, ss, nullptr, nullptr);
                continue;
            }
            double *tz = static_cast<double *>(tst->p), *ts = var ? static_cast<double *>(tcv->p) : nullptr;
            rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, tz, ts, nullptr, nullptr);
            if (rc) break;
            hipLaunchKernelGGL(sparse_pad_kernel, dim3((unsigned)sp_elementwise_grid(b.rows * K, ctx->n_cu)), dim3(256), 0, ctx->stream, tz, b.rows,
                               ke, K, 0, zs);
            if (var)
                hipLaunchKernelGGL(sparse_pad_kernel, dim3((unsigned)sp_elementwise_grid(b.rows * K * K, ctx->n_cu)), dim3(256), 0, ctx->stream, ts,
                                   b.rows, ke, K, 1, ss);
            if (hipGetLastError() != hipSuccess) rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
        }
        if (rc) break;
        const SpTopDims g = sp_top_dims(ctx, c, b, n_top, kappa, exclude_observed, nc);
        SpMixTopPtrs p{};
        p.row_ptr = static_cast<const int64_t *>(c.row_ptr->p);
        p.col = static_cast<const int32_t *>(c.col->p);
        p.cand = candidates ? static_cast<const int32_t *>(cd->p) : nullptr;
        p.comps = table_dev;
        p.resp = rp;
        p.states = stp;
        p.covs = cvp;
        p.ps = static_cast<double *>(g.final ? o.os->p : o.ps->p);
        p.pc = static_cast<int32_t *>(g.final ? o.oc->p : o.pc->p);
        p.nm = nm;
        p.cap = (int64_t)cap;
        if (launch_mix_topn(K, p, g, var, ctx->n_cu, ctx->stream) != hipSuccess) {
            rc = fail(PPCA_ERR_HIP, "mixture top-n launch failed");
            break;
        }
        rc = sp_top_finish(ctx, b, g, o, cols_host, scores_host);
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's buffer and `comps`)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "mixture top-n failed: %s", hipGetErrorString(e));
    return PPCA_OK;
}

// ------------------------------------------------------------------ held-out scoring
extern "C" int ppca_heldout_split_csr_host(int64_t n, const int64_t *row_ptr, const int32_t *col, double lo, double hi, uint64_t seed,
                                           int64_t row_offset, uint8_t *held_flag_out, int64_t *counts_out) {
    if (n < 0 || !row_ptr) return fail(PPCA_ERR_INVALID, "bad shape or null row_ptr");
    if (!(lo >= 0.0 && lo <= hi && hi <= 1.0)) return fail(PPCA_ERR_INVALID, "the range must satisfy 0 <= lo <= hi <= 1");
    if (row_offset < 0) return fail(PPCA_ERR_INVALID, "row_offset must be >= 0");
    if (row_ptr[0] != 0) return fail(PPCA_ERR_INVALID, "row_ptr must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(PPCA_ERR_INVALID, "row_ptr is not monotone at row %lld", (long long)i);
    if (row_ptr[n] > 0 && (!col || !held_flag_out)) return fail(PPCA_ERR_INVALID, "null col or output");
    int64_t held = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = row_key(seed, STREAM_HOLDOUT, (uint64_t)(row_offset + i));
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0) return fail(PPCA_ERR_INVALID, "column %d of row %lld is negative", col[e], (long long)i);
            const double u = u01_floor(row_word(key, (uint64_t)col[e]));
            const bool hold = u >= lo && u < hi;
            held_flag_out[e] = hold ? 1 : 0;
            held += hold ? 1 : 0;
        }
    }
    if (counts_out) {
        counts_out[0] = row_ptr[n] - held;
        counts_out[1] = held;
    }
    return PPCA_OK;
}

extern "C" int ppca_heldout_score_sparse(ppca_ctx *ctx, ppca_sparse *train, ppca_sparse *held, const ppca_model *model, double *totals_host,
                                         double *col_sums_host, double *per_row) {
    if (!held || !totals_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_check(ctx, train, model)) return rc;
    const SpCore &tc = *train->core, &hc = *held->core;
    if (tc.n != hc.n || tc.d != hc.d)
        return fail(PPCA_ERR_INVALID, "the train part (%lld x %d) and the held part (%lld x %d) differ in shape", (long long)tc.n, tc.d,
                    (long long)hc.n, hc.d);
    if (train->ctx->device != held->ctx->device) return fail(PPCA_ERR_INVALID, "the two datasets live on different devices");
    if (tc.block_rows != hc.block_rows)
        return fail(PPCA_ERR_INVALID, "the train part is tiled in blocks of %lld rows and the held part in blocks of %lld: build both with one "
                    "block_rows", (long long)tc.block_rows, (long long)hc.block_rows);
    USE_CTX(ctx);
    const int k = model->k, d = tc.d;
    const int64_t n = tc.n;
    static const int widths[3] = {4, 16, 64};
    BufRef st, cv, rows, sums, runpart;
    if (int rc = dev_alloc(sizeof(double) * (size_t)tc.max_rows * k, &st)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)tc.max_rows * k * k, &cv)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)n, &rows)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)SP_HELD_NO * d, &sums)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(hc.max_runs, 1) * SP_HELD_NO, &runpart)) return rc;
    double *stp = static_cast<double *>(st->p), *cvp = static_cast<double *>(cv->p), *rowv = static_cast<double *>(rows->p);
    double *colsum = static_cast<double *>(sums->p);
    HIP_TRY(hipMemsetAsync(rowv, 0, sizeof(double) * (size_t)n, ctx->stream));
    HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(double) * (size_t)SP_HELD_NO * d, ctx->stream));
    for (size_t bi = 0; bi < hc.blocks.size(); ++bi) {
        const SpBlock &tb = tc.blocks[bi], &hb = hc.blocks[bi];  // (the same rows: equal n and block_rows)
        if (hb.nnz == 0) continue;                               // nothing held in these rows: their scores stay 0
        if (int rc = sp_rows_of_block(ctx, train, tb, model, nullptr, stp, cvp, nullptr, nullptr)) return rc;
        for (int bin = 0; bin < 3; ++bin) {
            if (hb.nbin[bin] == 0) continue;
            SpHeldRowArgs a{};
            a.row_ptr = static_cast<const int64_t *>(hc.row_ptr->p);
            a.col = static_cast<const int32_t *>(hc.col->p);
            a.val = held->val();
            a.rows = static_cast<const int32_t *>(hb.rowlist->p) + hb.bin_off[bin];
            a.nrows = hb.nbin[bin];
            a.row0 = hb.row0;
            a.W = widths[bin];
            a.d = d;
            a.model = model->p();
            a.states = stp;
            a.covs = cvp;
            a.per_row = rowv;
            HIP_TRY(launch_held_row(k, a, sp_row_grid(a.nrows, a.W, ctx->n_cu), ctx->stream));
        }
        SpHeldColArgs a{};
        a.items = static_cast<const SpItem *>(hb.items->p);
        a.n_items = hb.n_items;
        a.trow = static_cast<const int32_t *>(hc.trow->p);
        a.tval = held->tval();
        a.w = train->w;
        a.row0 = hb.row0;
        a.states = stp;
        a.covs = cvp;
        a.model = model->p();
        a.d = d;
        a.colsum = colsum;
        a.runpart = static_cast<double *>(runpart->p);
        HIP_TRY(launch_held_col(k, a, ctx->n_cu, ctx->stream));
        if (hb.n_long > 0) {
            const int grid = (int)std::min<int64_t>((hb.n_long * SP_HELD_NO + 255) / 256, (int64_t)std::max(ctx->n_cu, 1) * 8);
            hipLaunchKernelGGL(sparse_held_fix_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream,
                               static_cast<const SpLong *>(hb.longs->p), hb.n_long, static_cast<const double *>(runpart->p), d, colsum);
            HIP_TRY(hipGetLastError());
        }
    }
    std::vector<double> cs((size_t)SP_HELD_NO * d);
    HIP_TRY(hipMemcpyAsync(cs.data(), colsum, sizeof(double) * cs.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (per_row) HIP_TRY(hipMemcpyAsync(per_row, rowv, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < SP_HELD_NO; ++q) {  // the column sums added in index order, as ppca_heldout_score's totals
        double s = 0.0;
        for (int j = 0; j < d; ++j) s += cs[(size_t)q * d + j];
        totals_host[q] = s;
    }
    totals_host[4] = (double)hc.nnz;
    totals_host[5] = (double)hc.nonempty_rows;
    if (col_sums_host) std::memcpy(col_sums_host, cs.data(), sizeof(double) * cs.size());
    return PPCA_OK;
}

// ------------------------------------------------------------------ factor analysis on row-compressed data
namespace {

// Enqueues the rescaling of sp under the device vectors abl = [a | b | l] (3 d): view (nullable) gets buffers of its own for
// val * a[col] in both orientations, on sp's core and weights; colsum (nullable, 3 x d, device) and rowsum (nullable, n, device) the
// sums.  The row kernel runs when a view or the row sums are wanted, the column kernel when a view or the column sums are.  No wait.
int sp_scale(ppca_ctx *ctx, const ppca_sparse *sp, const double *abl, ppca_sparse *view, double *colsum, double *rowsum) {
    const SpCore &c = *sp->core;
    static const int widths[3] = {4, 16, 64};
    double *ov = nullptr, *otv = nullptr;
    if (view) {
        view->ctx = sp->ctx;
        view->core = sp->core;
        view->wbuf = sp->wbuf;
        view->w = sp->w;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.nnz, 1), &view->vbuf)) return rc;
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.nnz, 1), &view->tvbuf)) return rc;
        ov = static_cast<double *>(view->vbuf->p);
        otv = static_cast<double *>(view->tvbuf->p);
    }
    BufRef runpart;
    if (colsum) {
        if (int rc = dev_alloc(sizeof(double) * (size_t)std::max<int64_t>(c.max_runs, 1) * SP_SCALE_NO, &runpart)) return rc;
        HIP_TRY(hipMemsetAsync(colsum, 0, sizeof(double) * (size_t)SP_SCALE_NO * c.d, ctx->stream));
    }
    for (const SpBlock &b : c.blocks) {
        if (ov || rowsum)
            for (int bin = 0; bin < 3; ++bin) {
                if (b.nbin[bin] == 0) continue;
                SpScaleRowArgs a{};
                a.row_ptr = static_cast<const int64_t *>(c.row_ptr->p);
                a.col = static_cast<const int32_t *>(c.col->p);
                a.val = sp->val();
                a.rows = static_cast<const int32_t *>(b.rowlist->p) + b.bin_off[bin];
                a.nrows = b.nbin[bin];
                a.row0 = b.row0;
                a.W = widths[bin];
                a.a = abl;
                a.l = abl + (size_t)2 * c.d;
                a.out_val = ov;
                a.rowsum = rowsum;
                hipLaunchKernelGGL(sparse_scale_row_kernel, dim3((unsigned)sp_row_grid(a.nrows, a.W, ctx->n_cu)), dim3(256), 0, ctx->stream, a);
                HIP_TRY(hipGetLastError());
            }
        if ((!otv && !colsum) || b.n_items == 0) continue;
        SpScaleColArgs a{};
        a.items = static_cast<const SpItem *>(b.items->p);
        a.n_items = b.n_items;
        a.trow = static_cast<const int32_t *>(c.trow->p);
        a.tval = sp->tval();
        a.w = sp->w;
        a.row0 = b.row0;
        a.a = abl;
        a.b = abl + c.d;
        a.d = c.d;
        a.out_tval = otv;
        a.colsum = colsum;
        a.runpart = colsum ? static_cast<double *>(runpart->p) : nullptr;
        constexpr int per_wg = 4 * (64 / SP_SCALE_GW);
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n_items + per_wg - 1) / per_wg, (int64_t)std::max(ctx->n_cu, 1) * 8));
        hipLaunchKernelGGL(sparse_scale_col_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        if (colsum && b.n_long > 0) {
            const int fgrid = (int)std::min<int64_t>((b.n_long * SP_SCALE_NO + 255) / 256, (int64_t)std::max(ctx->n_cu, 1) * 8);
            hipLaunchKernelGGL(sparse_scale_fix_kernel, dim3((unsigned)fgrid), dim3(256), 0, ctx->stream,
                               static_cast<const SpLong *>(b.longs->p), b.n_long, static_cast<const double *>(runpart->p), c.d, colsum);
            HIP_TRY(hipGetLastError());
        }
    }
    return PPCA_OK;
}

// [a | b | l] (b, l nullable = 0) on the device; h: the caller's staging vector, read until the stream's next synchronisation
int sp_upload_abl(ppca_ctx *ctx, int d, const double *a, const double *b, const double *l, std::vector<double> &h, BufRef *out) {
    h.assign((size_t)3 * d, 0.0);
    std::memcpy(h.data(), a, sizeof(double) * d);
    if (b) std::memcpy(h.data() + d, b, sizeof(double) * d);
    if (l) std::memcpy(h.data() + (size_t)2 * d, l, sizeof(double) * d);
    return sp_upload(ctx, h.data(), sizeof(double) * h.size(), out);
}

int sp_check_finite(const double *v, int d, const char *name) {
    if (v)
        for (int j = 0; j < d; ++j)
            if (!std::isfinite(v[j])) return fail(PPCA_ERR_INVALID, "%s[%d] is not a finite number", name, j);
    return PPCA_OK;
}

}  // namespace

extern "C" int ppca_scale_columns_sparse(ppca_ctx *ctx, ppca_sparse *sp, const double *a_host, const double *b_host, const double *l_host,
                                         ppca_sparse **out, double *col_sums_host, double *row_sums_host) {
    if (!ctx || !sp || !a_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (!out && !col_sums_host && !row_sums_host) return fail(PPCA_ERR_INVALID, "no output requested");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    const SpCore &c = *sp->core;
    if (int rc = sp_check_finite(a_host, c.d, "a")) return rc;
    if (int rc = sp_check_finite(b_host, c.d, "b")) return rc;
    if (int rc = sp_check_finite(l_host, c.d, "l")) return rc;
    USE_CTX(ctx);
    std::unique_ptr<ppca_sparse> view(out ? new ppca_sparse() : nullptr);
    std::vector<double> h;  // (read by the upload: alive until the synchronisation below)
    BufRef abl, cs, rs;
    int rc = sp_upload_abl(ctx, c.d, a_host, b_host, l_host, h, &abl);
    if (!rc && col_sums_host) rc = dev_alloc(sizeof(double) * (size_t)SP_SCALE_NO * c.d, &cs);
    if (!rc && row_sums_host && c.n > 0) rc = dev_alloc(sizeof(double) * (size_t)c.n, &rs);
    if (!rc)
        rc = sp_scale(ctx, sp, static_cast<const double *>(abl->p), view.get(), cs ? static_cast<double *>(cs->p) : nullptr,
                      rs ? static_cast<double *>(rs->p) : nullptr);
    if (!rc && cs && hipMemcpyAsync(col_sums_host, cs->p, sizeof(double) * (size_t)SP_SCALE_NO * c.d, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && rs && hipMemcpyAsync(row_sums_host, rs->p, sizeof(double) * (size_t)c.n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the upload reads `h`)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "scale pass failed: %s", hipGetErrorString(e));
    if (out) *out = view.release();
    return PPCA_OK;
}

extern "C" int ppca_fa_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, int32_t d, int32_t k, const double *noise, const double *transform,
                                      const double *mean, const double *min_noise, double *noise_out, double *transform_out,
                                      double *mean_out, double *llk_in) {
    if (!ctx || !sp || !noise || !mean || !noise_out || !mean_out || d < 1 || k < 0 || (k > 0 && (!transform || !transform_out)))
        return fail(PPCA_ERR_INVALID, "null argument");
    const SpCore &c = *sp->core;
    if (c.d != d) return fail(PPCA_ERR_INVALID, "dataset has %d dimensions but the model has output size %d", c.d, d);
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    if (k > SP_MAX_K)
        return fail(PPCA_ERR_UNSUPPORTED, "state size %d is not supported on sparse data: the kernels cover k <= %d", k, SP_MAX_K);
    if (c.n == 0) return fail(PPCA_ERR_EMPTY, "dataset is empty");
    for (int j = 0; j < d; ++j)
        if (!(noise[j] > 0.0) || !std::isfinite(noise[j])) return fail(PPCA_ERR_INVALID, "noise[%d] is not a positive finite number", j);
    USE_CTX(ctx);
    // the whitened model PPCAModel(1, A, mean~) and the whitening vectors a = 1 / s, b = mean / s, as ppca_fa_em_step forms them
    std::vector<double> inv((size_t)d), mw((size_t)d), A((size_t)d * k), sums((size_t)SP_SCALE_NO * d);
    for (int j = 0; j < d; ++j) {
        inv[j] = 1.0 / noise[j];
        mw[j] = mean[j] / noise[j];
        for (int b = 0; b < k; ++b) A[(int64_t)j * k + b] = transform[(int64_t)j * k + b] / noise[j];
    }
    if (int rc = sp_check_finite(inv.data(), d, "1 / noise")) return rc;
    if (int rc = sp_check_finite(mw.data(), d, "mean / noise")) return rc;
    ppca_model *m_raw = nullptr;
    if (int rc = ppca_model_create(ctx, d, k, 1.0, A.data(), mw.data(), &m_raw)) return rc;
    const std::unique_ptr<ppca_model, int (*)(ppca_model *)> m(m_raw, ppca_model_free);
    const StatsLayout L(d, m->k);
    if (int rc = ensure(ctx->stats, ctx->stats_cap, sizeof(double) * (size_t)L.len)) return rc;
    double *stats = static_cast<double *>(ctx->stats->p);
    ctx->stats_llk_at = -1;  // (the llk in the buffer is the whitened model's: ppca_em_last_llk does not apply)
    std::vector<double> h, hs((size_t)L.len);  // (h: read by the upload, alive until the synchronisation below)
    ppca_sparse view;  // (its two buffers go back to the context's block cache when it leaves scope)
    BufRef abl, cs;
    int rc = sp_upload_abl(ctx, d, inv.data(), mw.data(), nullptr, h, &abl);
    if (!rc) rc = dev_alloc(sizeof(double) * sums.size(), &cs);
    if (!rc) rc = sp_scale(ctx, sp, static_cast<const double *>(abl->p), &view, static_cast<double *>(cs->p), nullptr);
    if (!rc) rc = sp_accumulate(ctx, &view, m.get(), stats);
    if (!rc && hipMemcpyAsync(sums.data(), cs->p, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(hs.data(), stats, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // the one wait for the results (the upload reads `h`)
    if (rc) return rc;
    if (e != hipSuccess) return fail(PPCA_ERR_HIP, "FA step failed: %s", hipGetErrorString(e));
    if (int frc = ppca_fa_finalize_host(d, k, noise, transform, mean, hs.data(), sums.data() + (size_t)2 * d, min_noise, noise_out,
                                        transform_out, mean_out))
        return frc;
    if (llk_in) {
        double jac = 0.0;
        for (int j = 0; j < d; ++j) jac += hs[L.totals + j] * std::log(noise[j]);
        *llk_in = hs[L.scalars + SC_LLK] - jac;
    }
    return PPCA_OK;
}
