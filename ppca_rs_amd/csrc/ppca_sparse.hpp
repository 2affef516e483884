// ppca_sparse.hpp -- what the translation units of the row-compressed data path share (SparseDataset, DESIGN.md sections 4.20 - 4.31):
// ppca_sparse.hip (container, EM passes, llk / infer / predict), ppca_sparse_mix.hip, ppca_sparse_topn.hip, ppca_sparse_heldout.hip,
// ppca_sparse_fa.hip, ppca_sparse_robust.hip, ppca_sparse_hetero.hip and ppca_sparse_build.hip (the same container built on the device
// from CSR arrays that live there, and the split of such a handle).  Internal: not installed.
//
// Storage.  CSR on the device: row_ptr (int64, n + 1), col (int32, nnz, strictly increasing within a row), val (fp64, nnz).  Rows are
// cut into blocks of block_rows (fixed at construction: the records of a block stay under 1 GiB at k = 16).  Per block the constructor builds
//   - three row lists by row length m: m <= 16, m <= 64, longer (the bins of the row pass);
//   - the inverted index in CSC order (per column, the block's entries in ascending row): t_row (int32, row within the block) and
//     t_val, by a counting sort that is stable in row order (ppca_sparse_transpose_host);
//   - the work items of the column pass: a column with at most `segment` entries in the block is one item; a longer one is cut into
//     runs of exactly `segment` entries (the last one shorter), each an item that writes a partial.
// A ppca_sparse may carry buffers of its own for the values in both orientations (a values view, ppca_sparse_fa.hip: the pattern, row
// lists, index and work items are the core's), and every launcher reads the values through the handle.
//
// Every kernel of the path lives in namespace ppca_sp, as do the host functions that cross files; a helper of one file stays in that
// file's anonymous namespace.
#pragma once
#include <algorithm>
#include <functional>
#include <memory>
#include <vector>

#include "ppca_handles.hpp"
#include "ppca_sweep.hpp"

namespace ppca_sp {
using namespace ppca;
using namespace ppca_host;

constexpr int SP_MAX_K = 16;
constexpr int SP_SHORT = 16, SP_MID = 64;  // row-length bins: W = 4, 16, 64
constexpr int SP_SEGMENT = 512;            // default run length of a long column
constexpr int SP_NSCAL = 5;                // per-row scalar terms: w sq_err | w dev | w ell | w | non-empty
constexpr int SP_SCAL_ROWS = 1024;         // rows per workgroup of sparse_scal_kernel

template <class T>
T *dptr(const BufRef &b) { return static_cast<T *>(b->p); }

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
    BufRef rowlist_buf, items_buf, longs_buf;
    const int32_t *rowlist() const { return dptr<const int32_t>(rowlist_buf); }
    const SpItem *items() const { return dptr<const SpItem>(items_buf); }
    const SpLong *longs() const { return dptr<const SpLong>(longs_buf); }
};

struct SpCore {
    int64_t n = 0, nnz = 0, block_rows = 0, max_rows = 0, max_runs = 0, nonempty_rows = 0;
    int d = 0, segment = 0;
    BufRef row_ptr_buf, col_buf, val, trow_buf, tval;
    std::vector<SpBlock> blocks;
    std::vector<int32_t> empty;  // 1 = column without an entry
    double build_seconds = 0.0;
    const int64_t *row_ptr() const { return dptr<const int64_t>(row_ptr_buf); }
    const int32_t *col() const { return dptr<const int32_t>(col_buf); }
    const int32_t *trow() const { return dptr<const int32_t>(trow_buf); }
};

}  // namespace ppca_sp

struct ppca_sparse {
    ppca_ctx *ctx = nullptr;
    std::shared_ptr<ppca_sp::SpCore> core;
    BufRef wbuf;
    const double *w = nullptr;  // nullptr = all ones
    // A values view (ppca_scale_columns_sparse): buffers of its own for the values in CSR order and in
    // inverted-index order, on the pattern, row lists, index and work items of `core`.  Empty = the core's values.
    BufRef vbuf, tvbuf;
    const double *val() const { return ppca_sp::dptr<const double>(vbuf ? vbuf : core->val); }
    const double *tval() const { return ppca_sp::dptr<const double>(tvbuf ? tvbuf : core->tval); }
};

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

namespace ppca_sp {

// ------------------------------------------------------------------ device code of more than one file
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

// column sums (NO x d) of a long column += its runs' partials, added in run order: one thread per (column, sum).  Behind the column
// kernels of held-out scoring (NO = 4) and of the column rescaling (NO = 3).
template <int NO>
__global__ __launch_bounds__(256) void sparse_colsum_fix_kernel(const SpLong *longs, int64_t n_long, const double *runpart, int d, double *colsum) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_long * NO; t += stride) {
        const SpLong lc = longs[t / NO];
        const int q = (int)(t % NO);
        double s = 0.0;
        for (int r = 0; r < lc.nruns; ++r) s += runpart[(lc.first + r) * NO + q];
        colsum[(int64_t)q * d + lc.col] += s;
    }
}

// ------------------------------------------------------------------ host scaffolding
// workgroups for `units` of work at per_workgroup each: at least one, at most wgs_per_cu workgroups per compute unit (the kernels stride)
inline int sp_grid(int64_t units, int64_t per_workgroup, int n_cu, int wgs_per_cu) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((units + per_workgroup - 1) / per_workgroup, (int64_t)std::max(n_cu, 1) * wgs_per_cu));
}
// every kernel of the path runs in workgroups of 256 threads on the context's stream
template <class... P, class... A>
hipError_t sp_launch(void (*kernel)(P...), int grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, s, args...);
    return hipGetLastError();
}
// the one wait of an entry point whose asynchronous uploads read the caller's memory: reached on the error path too
inline int sp_finish(ppca_ctx *ctx, int rc, const char *what) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    return e == hipSuccess ? PPCA_OK : fail(PPCA_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}
// a row kernel over nrows rows in groups of W lanes: four waves of 64 / W rows per workgroup
inline int sp_row_grid(int64_t nrows, int W, int n_cu) { return sp_grid(nrows, 4 * (64 / W), n_cu, 8); }
// an element-wise or per-query-entry kernel over len outputs, one per thread
inline int sp_elementwise_grid(int64_t len, int n_cu) { return sp_grid(len, 256, n_cu, 16); }

// The row side of one block of sp: per non-empty row-length bin, the fields that every row kernel's arguments share (the CSR arrays,
// the bin's row list, its group width W) filled into a copy of `a`, then launch(a, grid of sp_row_grid).
template <class Args, class Launch>
int sp_for_bins(const ppca_ctx *ctx, const ppca_sparse *sp, const SpBlock &b, Args a, Launch launch) {
    static const int widths[3] = {4, 16, 64};
    a.row_ptr = sp->core->row_ptr();
    a.col = sp->core->col();
    a.val = sp->val();
    a.row0 = b.row0;
    for (int bin = 0; bin < 3; ++bin) {
        if (b.nbin[bin] == 0) continue;
        a.rows = b.rowlist() + b.bin_off[bin];
        a.nrows = b.nbin[bin];
        a.W = widths[bin];
        HIP_TRY(launch(a, sp_row_grid(a.nrows, a.W, ctx->n_cu)));
    }
    return PPCA_OK;
}

// The column side of one block of sp: the fields that every item kernel's arguments share (the work items, the inverted index, the
// runs' partials) filled into a copy of `a`, then item(a) and, where the block has columns cut into runs, fix().
template <class Args, class Item, class Fix>
int sp_col_pass(const ppca_sparse *sp, const SpBlock &b, double *runpart, Args a, Item item, Fix fix) {
    if (b.n_items == 0) return PPCA_OK;
    a.items = b.items();
    a.n_items = b.n_items;
    a.trow = sp->core->trow();
    a.tval = sp->tval();
    a.d = sp->core->d;
    a.runpart = runpart;
    HIP_TRY(item(a));
    if (b.n_long > 0) HIP_TRY(fix());
    return PPCA_OK;
}
template <int NO>
hipError_t sp_colsum_fix(const ppca_ctx *ctx, const SpBlock &b, const double *runpart, int d, double *colsum) {
    return sp_launch(sparse_colsum_fix_kernel<NO>, sp_grid(b.n_long * NO, 256, ctx->n_cu, 8), ctx->stream, b.longs(), b.n_long, runpart, d, colsum);
}

// ------------------------------------------------------------------ host functions that cross files
// ppca_sparse.hip
int sp_upload(ppca_ctx *ctx, const void *src, size_t bytes, BufRef *out);
int sp_check(const ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model);
// the query pattern of a predict call; *nq = its entries (0: nothing to do, the outputs may be null)
int sp_check_query(const SpCore &c, const int64_t *query_row_ptr, const int32_t *query_col, const double *mean_host, const double *var_host,
                   int64_t *nq);
// the row pass (sparse_row_kernel<k>) over one block: outputs, all nullable, indexed by the row within the block
int sp_rows_of_block(ppca_ctx *ctx, const ppca_sparse *sp, const SpBlock &b, const ppca_model *model, double *llks, double *states, double *covs,
                     double *rec, double *rscal);
// ppca_sparse_predict behind its checks of (ctx, sp, model): the query's checks and upload, then per block with a query entry
// rows_of_block(block, states, covs) -- the caller's row pass into one block's scratch -- and sparse_predict_kernel, the download, one wait
typedef std::function<int(const SpBlock &, double *, double *)> SpRowPass;
int sp_predict(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, const int64_t *query_row_ptr, const int32_t *query_col,
               double *mean_host, double *var_host, const SpRowPass &rows_of_block);
// the scratch of sp_accumulate at state size k: one block's records and scalar terms, the scalars' partials, the runs' partials
struct SpAccScratch {
    BufRef rec, rscal, spart, runpart;
};
int sp_acc_scratch(const SpCore &c, int k, SpAccScratch *s);
// the packed statistics of sp under model; scratch: nullptr = taken here; the mixture step hands in ONE, sized for its largest state
// size, taken before its first launch
int sp_accumulate(ppca_ctx *ctx, const ppca_sparse *sp, const ppca_model *model, double *stats, const SpAccScratch *scratch = nullptr);

// ppca_sparse_mix.hip
int sp_mix_check(const ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t nm);
struct SpMixDev {
    double *llk, *u, *lse, *logpost;
    MixAux ax;
};
// every block the posteriors need, in the context's mixture scratch (kept across iterations)
int sp_mix_blocks(ppca_ctx *ctx, int64_t n, int nm, bool want_logpost, SpMixDev *m);
// ell of every component, then u = ln w + log posterior, the rows' mixture log-density and (nullable) the log posteriors
int sp_mix_posteriors(ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int nm, const SpMixDev &m);

}  // namespace ppca_sp
