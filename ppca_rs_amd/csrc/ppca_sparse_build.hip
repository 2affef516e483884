// ppca_sparse_build.hip -- the container of row-compressed data built on the device: ppca_from_device_sparse
// borrows CSR arrays that already live there and builds the row lists, the inverted index and the work items of ppca_sparse.hpp with
// kernels; ppca_heldout_split_sparse is the hold-out split of ppca_heldout_split_csr_host on such a handle, its two parts built the
// same way; ppca_index_to_host_sparse hands the index of a handle from either constructor back.  The oracle is the host constructor
// (ppca_sparse_from_host, ppca_sparse.hip): every array and count built here equals what it builds from the same arrays, integer for
// integer.  Nothing here computes in floating point: a value is tested for finiteness and copied, bits kept.
//
// build_rowptr_kernel / build_entry_kernel  the host constructor's rules.  A violation is reported as the lowest offending row, an
//     integer minimum over the violating rows or entries: the report does not depend on the grid.  The host then reads that one row and
//     words the message as the host constructor does.
// build_scan_tile_kernel<T> / build_scan_add_kernel<T>  an exclusive prefix sum of integers in place, 2048 elements per workgroup, the
//     workgroups' totals scanned by the same kernels (sb_scan).  Behind the row lists, the column offsets, the work items, each
//     pass of the sort and the split.
// build_row_flags_kernel / build_rowlist_kernel  the three row lists of a block: the flags [bin][row] laid end to end and scanned give
//     every row its slot in the block's list, each bin in ascending row.
// build_colcount_kernel / build_item_counts_kernel / build_items_kernel  the column counts of a block (integer atomics: a count does
//     not depend on the order), their scan (the column offsets), per column its number of items, long columns and runs, their scan,
//     and the items and long columns written at those slots: the host loop's order, dest slots and run lengths.
// build_sort_hist_kernel / build_sort_scatter_kernel  the inverted index: a least-significant-digit radix sort of the block's entries
//     by column, 8 bits a pass, stable, so that the entries of a column stay in ascending row -- the counting sort of
//     sp_transpose_block.  A pass counts the digits of every tile of 4096 entries, scans the counts in (digit, tile) order and scatters
//     tile by tile: a tile goes through its workgroup in chunks of 256 entries, a lane's rank among its wave's lanes of equal digit
//     comes from eight ballots, the waves' counts are added in wave order.  No cursor is bumped by an atomic.  The first pass reads
//     its keys from the CSR and finds each entry's row by bisection of row_ptr; the last one writes t_row and t_val.
// split_flag_kernel<T> / split_compact_kernel<T> / split_rowptr_kernel<T>  the split: a flag per entry from the word of the dense
//     split, a scan, and the entries and row offsets of the two parts written at the scanned slots.
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>

#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

constexpr int SB_TILE = 4096;       // entries of a sort tile: 16 chunks of 256
constexpr int SB_SCAN_TILE = 2048;  // elements of a scan tile: 8 per thread
typedef unsigned long long sb_u64;
constexpr sb_u64 SB_NONE = ~0ull;

// ------------------------------------------------------------------ validation
// out[0] = 1 iff row_ptr[0] != 0 | out[1] = the lowest row with row_ptr[i + 1] < row_ptr[i] | out[2] = the lowest row with more than d
// entries | out[3] = the rows with an entry.  out[1], out[2]: SB_NONE on entry.
__global__ __launch_bounds__(256) void build_rowptr_kernel(const int64_t *row_ptr, int64_t n, int d, sb_u64 *out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (first == 0 && row_ptr[0] != 0) out[0] = 1;
    sb_u64 live = 0;
    for (int64_t i = first; i < n; i += stride) {
        const int64_t m = row_ptr[i + 1] - row_ptr[i];
        if (m < 0) atomicMin(&out[1], (sb_u64)i);
        if (m > d) atomicMin(&out[2], (sb_u64)i);
        live += m > 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) live += __shfl_xor(live, o, 64);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&out[3], live);
}

// *bad_row = the lowest row with a column outside [0, d), a column not above its predecessor in the row, or a value that is not finite
// (row_ptr: monotone from 0 to nnz, checked before; n >= 1).  An entry's row is looked up where a rule may be broken, not before.
__global__ __launch_bounds__(256) void build_entry_kernel(const int64_t *row_ptr, const int32_t *col, const double *val, int64_t n, int d,
                                                          int64_t nnz, sb_u64 *bad_row) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int c = col[e];
        bool bad = c < 0 || c >= d || !isfinite(val[e]);
        const bool look = bad || (e > 0 && c <= col[e - 1]);
        if (!look) continue;
        const int64_t r = query_row(row_ptr, e, 0, n);
        bad = bad || row_ptr[r] != e;  // (not the row's first entry: its predecessor belongs to the same row)
        if (bad) atomicMin(bad_row, (sb_u64)r);
    }
}

// bounds[b] = row_ptr[min(n, b block_rows)], b = 0 .. n_blocks
__global__ __launch_bounds__(256) void build_bounds_kernel(const int64_t *row_ptr, int64_t n, int64_t block_rows, int64_t n_blocks,
                                                           int64_t *bounds) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= n_blocks; b += stride) {
        const int64_t r = b * block_rows < n ? b * block_rows : n;
        bounds[b] = row_ptr[r];
    }
}

// ------------------------------------------------------------------ the scan
// a[i] <- a[t SB_SCAN_TILE] + ... + a[i - 1] within tile t, sums[t] <- the tile's total
template <class T>
__global__ __launch_bounds__(256) void build_scan_tile_kernel(T *a, int64_t n, T *sums) {
    __shared__ T wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t ntiles = (n + SB_SCAN_TILE - 1) / SB_SCAN_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (uniform over the workgroup)
        const int64_t base = t * SB_SCAN_TILE + tid * 8;
        T v[8], s = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const T x = base + q < n ? a[base + q] : (T)0;
            v[q] = s;
            s += x;
        }
        T inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const T y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        T before = inc - s;
        for (int u = 0; u < w; ++u) before += wsum[u];
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (base + q < n) a[base + q] = v[q] + before;
        if (tid == 0) sums[t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}
// a[i] += sums[i / SB_SCAN_TILE] (the scanned totals), a[n] <- sums[ntiles], the grand total
template <class T>
__global__ __launch_bounds__(256) void build_scan_add_kernel(T *a, int64_t n, const T *sums, int64_t ntiles) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = first; i < n; i += stride) a[i] += sums[i / SB_SCAN_TILE];
    if (first == 0) a[n] = sums[ntiles];
}

// ------------------------------------------------------------------ row lists
__device__ __forceinline__ int sb_bin(int64_t m) { return m <= SP_SHORT ? 0 : m <= SP_MID ? 1 : 2; }
// flags[bin rows + i] = 1 iff row i of the block belongs to `bin`
__global__ __launch_bounds__(256) void build_row_flags_kernel(const int64_t *row_ptr, int64_t row0, int64_t rows, int32_t *flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < 3 * rows; q += stride) {
        const int64_t i = q % rows;
        flags[q] = sb_bin(row_ptr[row0 + i + 1] - row_ptr[row0 + i]) == (int)(q / rows) ? 1 : 0;
    }
}
// slot: the scanned flags.  The bins lie end to end in the list, so the scan over [bin][row] is the slot itself.
__global__ __launch_bounds__(256) void build_rowlist_kernel(const int64_t *row_ptr, int64_t row0, int64_t rows, const int32_t *slot,
                                                            int32_t *rowlist) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < 3 * rows; q += stride) {
        const int64_t i = q % rows;
        if (sb_bin(row_ptr[row0 + i + 1] - row_ptr[row0 + i]) == (int)(q / rows)) rowlist[slot[q]] = (int32_t)i;
    }
}

// ------------------------------------------------------------------ column counts, work items
__global__ __launch_bounds__(256) void build_colcount_kernel(const int32_t *col, int64_t nb, int32_t *cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) atomicAdd(&cnt[col[i]], 1);
}
// ic[j] = the items of column j | ic[d + j] = 1 iff it is cut into runs | ic[2 d + j] = its runs (cp: the block's column offsets)
__global__ __launch_bounds__(256) void build_item_counts_kernel(const int32_t *cp, int d, int seg, int64_t *ic) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += stride) {
        const int64_t cnt = cp[j + 1] - cp[j], nruns = (cnt + seg - 1) / seg;
        ic[j] = cnt <= seg ? (cnt > 0 ? 1 : 0) : nruns;
        ic[d + j] = cnt > seg ? 1 : 0;
        ic[2 * (int64_t)d + j] = cnt > seg ? nruns : 0;
    }
}
// ic: scanned.  The items, long columns and run slots of column j start where the columns before it end: the order of the host loop.
__global__ __launch_bounds__(256) void build_items_kernel(const int32_t *cp, const int64_t *ic, int d, int seg, int64_t e0, SpItem *items,
                                                          SpLong *longs, int32_t *seen) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < d; j += stride) {
        const int64_t cnt = cp[j + 1] - cp[j];
        if (cnt == 0) continue;
        seen[j] = 1;
        const int64_t at = ic[j], start = e0 + cp[j];
        if (cnt <= seg) {
            items[at] = SpItem{start, -1, (int32_t)j, (int32_t)cnt};
        } else {
            const int64_t nruns = (cnt + seg - 1) / seg, run0 = ic[2 * (int64_t)d + j] - ic[2 * (int64_t)d];
            longs[ic[d + j] - ic[d]] = SpLong{run0, (int32_t)j, (int32_t)nruns};
            for (int64_t r = 0; r < nruns; ++r) {
                const int64_t left = cnt - r * seg;
                items[at + r] = SpItem{start + r * seg, run0 + r, (int32_t)j, (int32_t)(left < seg ? left : seg)};
            }
        }
    }
}
// out[0..2] = slot[rows], slot[2 rows], slot[3 rows] (the ends of the three row lists) | out[3..5] = the block's items, long columns, runs
__global__ void build_summary_kernel(const int32_t *slot, int64_t rows, const int64_t *ic, int d, int64_t *out) {
    const int t = threadIdx.x;
    if (t < 3) out[t] = slot[(t + 1) * rows];
    if (t >= 3 && t < 6) out[t] = ic ? ic[(int64_t)(t - 2) * d] - ic[(int64_t)(t - 3) * d] : 0;
}

// ------------------------------------------------------------------ the sort
struct SbSortArgs {
    const int64_t *row_ptr;  // the CSR: keys and rows of the first pass, values of the last
    const int32_t *col;
    const double *val;
    int64_t e0, row0, rows, nb, ntiles;  // the block's first entry, first row, rows, entries; its sort tiles
    int shift;
    const int32_t *kin, *rin, *sin;  // a later pass: key, row within the block and source entry (relative to e0), in the order so far
    int32_t *kout, *rout, *sout;     // (the last pass: rout = the block's t_row, no kout, no sout)
    double *tval;                    // the last pass: the block's t_val
    int32_t *hist;                   // [digit][tile]
};

template <bool FIRST>
__global__ __launch_bounds__(256) void build_sort_hist_kernel(SbSortArgs a) {
    __shared__ int cnt[256];
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {  // (uniform over the workgroup)
        cnt[tid] = 0;
        __syncthreads();
        for (int c = 0; c < SB_TILE / 256; ++c) {
            const int64_t i = t * SB_TILE + c * 256 + tid;
            if (i < a.nb) {
                const int key = FIRST ? a.col[a.e0 + i] : a.kin[i];
                atomicAdd(&cnt[(key >> a.shift) & 255], 1);
            }
        }
        __syncthreads();
        a.hist[(int64_t)tid * a.ntiles + t] = cnt[tid];
        __syncthreads();
    }
}

// hist: scanned, so hist[digit][tile] is where the tile's first entry of that digit goes
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void build_sort_scatter_kernel(SbSortArgs a) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    __shared__ int64_t span[2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {  // (uniform over the workgroup)
        const int64_t i0 = t * SB_TILE, i1 = i0 + SB_TILE < a.nb ? i0 + SB_TILE : a.nb;
        base[tid] = a.hist[(int64_t)tid * a.ntiles + t];
#pragma unroll
        for (int u = 0; u < 4; ++u) wcnt[u][tid] = 0;
        if (FIRST && tid < 2) span[tid] = query_row(a.row_ptr, a.e0 + (tid == 0 ? i0 : i1 - 1), a.row0, a.rows);  // the tile's rows
        __syncthreads();
        const int64_t rlo = FIRST ? span[0] : 0, rcnt = FIRST ? span[1] - span[0] + 1 : 0;
        for (int64_t c0 = i0; c0 < i1; c0 += 256) {  // (uniform) the chunks in order, the waves of a chunk in order, the lanes in order
            const int64_t i = c0 + tid;
            const bool live = i < i1;
            int key = 0, row = 0, src = 0;
            if (live) {
                if (FIRST) {
                    key = a.col[a.e0 + i];
                    row = (int)(query_row(a.row_ptr, a.e0 + i, rlo, rcnt) - a.row0);
                    src = (int)i;
                } else {
                    key = a.kin[i];
                    row = a.rin[i];
                    src = a.sin[i];
                }
            }
            const int dg = (key >> a.shift) & 255;
            sb_u64 same = __ballot(live);  // the wave's live lanes of this lane's digit
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (dg >> b) & 1;
                const sb_u64 bb = __ballot(bit);
                same &= bit ? bb : ~bb;
            }
            const int rank = __popcll(same & ((1ull << lane) - 1ull));
            if (live && rank == 0) wcnt[w][dg] = __popcll(same);
            __syncthreads();
            if (live) {
                int pos = base[dg] + rank;
                for (int u = 0; u < w; ++u) pos += wcnt[u][dg];
                a.rout[pos] = row;
                if (LAST) {
                    a.tval[pos] = a.val[a.e0 + src];
                } else {
                    a.kout[pos] = key;
                    a.sout[pos] = src;
                }
            }
            __syncthreads();
            base[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
#pragma unroll
            for (int u = 0; u < 4; ++u) wcnt[u][tid] = 0;
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ the split
// held[e] = 1 iff entry e draws lo <= u < hi: the word of holdout_kernel and of ppca_heldout_split_csr_host
template <class T>
__global__ __launch_bounds__(256) void split_flag_kernel(const int64_t *row_ptr, const int32_t *col, int64_t n, int64_t nnz, double lo, double hi,
                                                         uint64_t seed, int64_t row_offset, T *held) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t r = query_row(row_ptr, e, 0, n);
        const uint64_t key = row_key(seed, STREAM_HOLDOUT, (uint64_t)(row_offset + r));
        const double u = u01_floor(row_word(key, (uint64_t)col[e]));
        held[e] = (u >= lo && u < hi) ? 1 : 0;
    }
}
// at: the scanned flags (nnz + 1).  Entry e goes to slot at[e] of the held part or to slot e - at[e] of the train part.
template <class T>
__global__ __launch_bounds__(256) void split_compact_kernel(const int32_t *col, const double *val, int64_t nnz, const T *at, int32_t *tcol,
                                                            double *tval, int32_t *hcol, double *hval) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int64_t h = (int64_t)at[e];
        if ((int64_t)at[e + 1] > h) {
            hcol[h] = col[e];
            hval[h] = val[e];
        } else {
            tcol[e - h] = col[e];
            tval[e - h] = val[e];
        }
    }
}
template <class T>
__global__ __launch_bounds__(256) void split_rowptr_kernel(const int64_t *row_ptr, int64_t n, const T *at, int64_t *tptr, int64_t *hptr) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
        const int64_t e = row_ptr[i], h = (int64_t)at[e];
        hptr[i] = h;
        tptr[i] = e - h;
    }
}

}  // namespace ppca_sp

namespace {

// (sp_default_block_rows of ppca_sparse.hip, which keeps it to itself: the records of a block stay under 1 GiB at k = 16)
int64_t sb_default_block_rows() { return ((int64_t)1 << 30) / (8 * (SP_MAX_K + 1 + SP_MAX_K * (SP_MAX_K + 1) / 2)); }

int sb_alloc(size_t bytes, BufRef *out) { return dev_alloc(std::max<size_t>(bytes, 8), out); }

// elements of scratch that sb_scan of n elements takes: the tiles' totals of every level, each with its grand total behind it
int64_t sb_scan_scratch(int64_t n) {
    int64_t len = 0;
    while (n > SB_SCAN_TILE) {
        n = (n + SB_SCAN_TILE - 1) / SB_SCAN_TILE;
        len += n + 1;
    }
    return len;
}
// a (n + 1 elements, the last one not read): a[i] <- a[0] + ... + a[i - 1], a[n] <- the total.  scratch: sb_scan_scratch(n) elements.
template <class T>
int sb_scan(ppca_ctx *ctx, T *a, int64_t n, T *scratch) {
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(a, 0, sizeof(T), ctx->stream));
        return PPCA_OK;
    }
    const int64_t ntiles = (n + SB_SCAN_TILE - 1) / SB_SCAN_TILE;
    if (ntiles == 1) {
        HIP_TRY(sp_launch(build_scan_tile_kernel<T>, 1, ctx->stream, a, n, a + n));
        return PPCA_OK;
    }
    HIP_TRY(sp_launch(build_scan_tile_kernel<T>, sp_grid(ntiles, 1, ctx->n_cu, 8), ctx->stream, a, n, scratch));
    if (int rc = sb_scan(ctx, scratch, ntiles, scratch + ntiles + 1)) return rc;
    HIP_TRY(sp_launch(build_scan_add_kernel<T>, sp_elementwise_grid(n, ctx->n_cu), ctx->stream, a, n, (const T *)scratch, ntiles));
    return PPCA_OK;
}

int sb_passes(int d) { return d <= (1 << 8) ? 1 : d <= (1 << 16) ? 2 : d <= (1 << 24) ? 3 : 4; }

// The message of the host constructor for row r, the lowest one that breaks a rule of the entries: the row comes to the host (at most d
// entries; a longer one is the violation).
int sb_report_row(ppca_ctx *ctx, const int64_t *row_ptr, const int32_t *col, const double *val, int32_t d, int64_t r) {
    int64_t rp[2];
    HIP_TRY(hipMemcpyAsync(rp, row_ptr + r, sizeof(rp), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t m = rp[1] - rp[0];
    if (m > d) return fail(PPCA_ERR_INVALID, "row %lld has more entries than columns", (long long)r);
    std::vector<int32_t> c((size_t)m);
    std::vector<double> v((size_t)m);
    HIP_TRY(hipMemcpyAsync(c.data(), col + rp[0], sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(v.data(), val + rp[0], sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t e = 0; e < m; ++e) {
        if (c[e] < 0 || c[e] >= d) return fail(PPCA_ERR_INVALID, "column %d of row %lld is outside [0, %d)", c[e], (long long)r, d);
        if (e > 0 && c[e] <= c[e - 1]) return fail(PPCA_ERR_INVALID, "columns of row %lld are not strictly increasing", (long long)r);
        if (!std::isfinite(v[e])) return fail(PPCA_ERR_INVALID, "value %lld of row %lld is not finite", (long long)e, (long long)r);
    }
    return fail(PPCA_ERR_INVALID, "row %lld breaks the format", (long long)r);
}

// What one build takes once and every block uses: sized for the largest block.
struct SbScratch {
    BufRef slot, cp, ic, hist, scan, summary, pay[6];
    int32_t *key[2] = {nullptr, nullptr}, *row[2] = {nullptr, nullptr}, *src[2] = {nullptr, nullptr};
};

int sb_scratch(const SpCore &c, int64_t max_nnz, SbScratch *s) {
    const int64_t d = c.d, tiles = (max_nnz + SB_TILE - 1) / SB_TILE;
    const int64_t longest = std::max(std::max<int64_t>(3 * c.max_rows, 3 * d), 256 * tiles);
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)(3 * c.max_rows + 1), &s->slot)) return rc;
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)(d + 1), &s->cp)) return rc;
    if (int rc = sb_alloc(sizeof(int64_t) * (size_t)(3 * d + 1), &s->ic)) return rc;
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)(256 * tiles + 1), &s->hist)) return rc;
    if (int rc = sb_alloc(sizeof(int64_t) * (size_t)sb_scan_scratch(longest), &s->scan)) return rc;
    if (int rc = sb_alloc(sizeof(int64_t) * 6, &s->summary)) return rc;
    const int sets = std::min(sb_passes(c.d) - 1, 2);  // a pass that is not the last writes (key, row, source); they ping-pong
    for (int i = 0; i < 3 * sets; ++i)
        if (int rc = sb_alloc(sizeof(int32_t) * (size_t)max_nnz, &s->pay[i])) return rc;
    for (int i = 0; i < sets; ++i) {
        s->key[i] = dptr<int32_t>(s->pay[3 * i]);
        s->row[i] = dptr<int32_t>(s->pay[3 * i + 1]);
        s->src[i] = dptr<int32_t>(s->pay[3 * i + 2]);
    }
    return PPCA_OK;
}

// t_row and t_val of block b
int sb_sort_block(ppca_ctx *ctx, const SpCore &c, const SpBlock &b, const SbScratch &s) {
    const int passes = sb_passes(c.d);
    SbSortArgs a{};
    a.row_ptr = c.row_ptr();
    a.col = c.col();
    a.val = dptr<const double>(c.val);
    a.e0 = b.e0;
    a.row0 = b.row0;
    a.rows = b.rows;
    a.nb = b.nnz;
    a.ntiles = (b.nnz + SB_TILE - 1) / SB_TILE;
    a.hist = dptr<int32_t>(s.hist);
    const int grid = sp_grid(a.ntiles, 1, ctx->n_cu, 8);
    for (int p = 0; p < passes; ++p) {
        const bool first = p == 0, last = p == passes - 1;
        a.shift = 8 * p;
        if (!first) {
            a.kin = s.key[(p - 1) & 1];
            a.rin = s.row[(p - 1) & 1];
            a.sin = s.src[(p - 1) & 1];
        }
        if (last) {
            a.kout = a.sout = nullptr;
            a.rout = dptr<int32_t>(c.trow_buf) + b.e0;
            a.tval = dptr<double>(c.tval) + b.e0;
        } else {
            a.kout = s.key[p & 1];
            a.rout = s.row[p & 1];
            a.sout = s.src[p & 1];
        }
        HIP_TRY(first ? sp_launch(build_sort_hist_kernel<true>, grid, ctx->stream, a) : sp_launch(build_sort_hist_kernel<false>, grid, ctx->stream, a));
        if (int rc = sb_scan(ctx, a.hist, 256 * a.ntiles, reinterpret_cast<int32_t *>(dptr<int64_t>(s.scan)))) return rc;
        if (first && last)
            HIP_TRY(sp_launch(build_sort_scatter_kernel<true, true>, grid, ctx->stream, a));
        else if (first)
            HIP_TRY(sp_launch(build_sort_scatter_kernel<true, false>, grid, ctx->stream, a));
        else if (last)
            HIP_TRY(sp_launch(build_sort_scatter_kernel<false, true>, grid, ctx->stream, a));
        else
            HIP_TRY(sp_launch(build_sort_scatter_kernel<false, false>, grid, ctx->stream, a));
    }
    return PPCA_OK;
}

// The core of a dataset whose CSR arrays (rp: n + 1, col and val: rp[n]) are on the device: validation (check_entries = 0: the rules of
// row_ptr alone, for arrays this file has just written), then everything ppca_sparse_from_host builds, array for array.
int sb_build_core(ppca_ctx *ctx, int64_t n, int32_t d, const BufRef &rp, const BufRef &colb, const BufRef &valb, int64_t block_rows,
                  int32_t segment, int check_entries, std::shared_ptr<SpCore> *out) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = ctx->stream;
    auto core = std::make_shared<SpCore>();
    core->n = n;
    core->d = d;
    core->block_rows = block_rows > 0 ? block_rows : sb_default_block_rows();
    core->segment = segment > 0 ? segment : SP_SEGMENT;
    core->row_ptr_buf = rp;
    core->col_buf = colb;
    core->val = valb;
    const int64_t *row_ptr = core->row_ptr();
    const int32_t *col = core->col();
    const double *val = dptr<const double>(core->val);

    // validation and counts
    BufRef chk;
    if (int rc = sb_alloc(sizeof(sb_u64) * 4, &chk)) return rc;
    sb_u64 *chkp = dptr<sb_u64>(chk), h[4];
    int64_t nnz = 0;
    HIP_TRY(hipMemsetAsync(chkp, 0, sizeof(sb_u64) * 4, st));
    HIP_TRY(hipMemsetAsync(chkp + 1, 0xFF, sizeof(sb_u64) * 2, st));
    HIP_TRY(sp_launch(build_rowptr_kernel, sp_elementwise_grid(n, ctx->n_cu), st, row_ptr, n, (int)d, chkp));
    HIP_TRY(hipMemcpyAsync(h, chkp, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&nnz, row_ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0]) return fail(PPCA_ERR_INVALID, "row_ptr must start at 0");
    if (h[1] != SB_NONE) return fail(PPCA_ERR_INVALID, "row_ptr is not monotone at row %lld", (long long)h[1]);
    if (nnz > 0 && (!col || !val)) return fail(PPCA_ERR_INVALID, "null col or val");
    if (check_entries && nnz > 0) {
        HIP_TRY(sp_launch(build_entry_kernel, sp_elementwise_grid(nnz, ctx->n_cu), st, row_ptr, col, val, n, (int)d, nnz, chkp + 2));
        HIP_TRY(hipMemcpyAsync(h + 2, chkp + 2, sizeof(sb_u64), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (h[2] != SB_NONE) return sb_report_row(ctx, row_ptr, col, val, d, (int64_t)h[2]);
    core->nnz = nnz;
    core->nonempty_rows = (int64_t)h[3];
    core->empty.assign((size_t)d, 1);

    // the blocks: row_ptr at their boundaries
    const int64_t br = core->block_rows, n_blocks = (n + br - 1) / br;
    int64_t max_nnz = 0;
    if (n_blocks > 0) {
        BufRef bnd;
        if (int rc = sb_alloc(sizeof(int64_t) * (size_t)(n_blocks + 1), &bnd)) return rc;
        std::vector<int64_t> bounds((size_t)n_blocks + 1);
        HIP_TRY(sp_launch(build_bounds_kernel, sp_elementwise_grid(n_blocks + 1, ctx->n_cu), st, row_ptr, n, br, n_blocks, dptr<int64_t>(bnd)));
        HIP_TRY(hipMemcpyAsync(bounds.data(), bnd->p, sizeof(int64_t) * bounds.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int64_t i = 0; i < n_blocks; ++i) {
            SpBlock b;
            b.row0 = i * br;
            b.rows = std::min(n, b.row0 + br) - b.row0;
            b.e0 = bounds[(size_t)i];
            b.nnz = bounds[(size_t)i + 1] - b.e0;
            if (b.nnz > INT32_MAX) return fail(PPCA_ERR_INVALID, "a block of %lld rows holds more than 2^31 entries: lower block_rows", (long long)b.rows);
            core->max_rows = std::max(core->max_rows, b.rows);
            max_nnz = std::max(max_nnz, b.nnz);
            core->blocks.push_back(b);
        }
    }
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)nnz, &core->trow_buf)) return rc;
    if (int rc = sb_alloc(sizeof(double) * (size_t)nnz, &core->tval)) return rc;
    if (n_blocks > 0) {
        SbScratch s;
        BufRef seen;
        if (int rc = sb_scratch(*core, max_nnz, &s)) return rc;
        if (int rc = sb_alloc(sizeof(int32_t) * (size_t)d, &seen)) return rc;
        HIP_TRY(hipMemsetAsync(seen->p, 0, sizeof(int32_t) * (size_t)d, st));
        int32_t *slot = dptr<int32_t>(s.slot), *cp = dptr<int32_t>(s.cp);
        int64_t *ic = dptr<int64_t>(s.ic), *scan = dptr<int64_t>(s.scan), *summary = dptr<int64_t>(s.summary);
        const int seg = core->segment;
        for (SpBlock &b : core->blocks) {
            // the row lists
            if (int rc = sb_alloc(sizeof(int32_t) * (size_t)b.rows, &b.rowlist_buf)) return rc;
            const int rgrid = sp_elementwise_grid(3 * b.rows, ctx->n_cu), dgrid = sp_elementwise_grid(d, ctx->n_cu);
            HIP_TRY(sp_launch(build_row_flags_kernel, rgrid, st, row_ptr, b.row0, b.rows, slot));
            if (int rc = sb_scan(ctx, slot, 3 * b.rows, reinterpret_cast<int32_t *>(scan))) return rc;
            HIP_TRY(sp_launch(build_rowlist_kernel, rgrid, st, row_ptr, b.row0, b.rows, (const int32_t *)slot, dptr<int32_t>(b.rowlist_buf)));
            if (b.nnz > 0) {
                // the column offsets, the counts of the work items, the index
                HIP_TRY(hipMemsetAsync(cp, 0, sizeof(int32_t) * (size_t)(d + 1), st));
                HIP_TRY(sp_launch(build_colcount_kernel, sp_elementwise_grid(b.nnz, ctx->n_cu), st, col + b.e0, b.nnz, cp));
                if (int rc = sb_scan(ctx, cp, (int64_t)d, reinterpret_cast<int32_t *>(scan))) return rc;
                HIP_TRY(sp_launch(build_item_counts_kernel, dgrid, st, (const int32_t *)cp, (int)d, seg, ic));
                if (int rc = sb_scan(ctx, ic, 3 * (int64_t)d, scan)) return rc;
            }
            hipLaunchKernelGGL(build_summary_kernel, dim3(1), dim3(64), 0, st, (const int32_t *)slot, b.rows, b.nnz > 0 ? (const int64_t *)ic : nullptr,
                               (int)d, summary);
            HIP_TRY(hipGetLastError());
            int64_t sum[6];
            HIP_TRY(hipMemcpyAsync(sum, summary, sizeof(sum), hipMemcpyDeviceToHost, st));
            if (b.nnz > 0)
                if (int rc = sb_sort_block(ctx, *core, b, s)) return rc;  // (queued behind the copy: it runs while the host waits)
            HIP_TRY(hipStreamSynchronize(st));
            b.bin_off[0] = 0;
            b.bin_off[1] = sum[0];
            b.bin_off[2] = sum[1];
            b.nbin[0] = sum[0];
            b.nbin[1] = sum[1] - sum[0];
            b.nbin[2] = sum[2] - sum[1];
            b.n_items = sum[3];
            b.n_long = sum[4];
            b.n_runs = sum[5];
            if (int rc = sb_alloc(sizeof(SpItem) * (size_t)b.n_items, &b.items_buf)) return rc;
            if (int rc = sb_alloc(sizeof(SpLong) * (size_t)b.n_long, &b.longs_buf)) return rc;
            if (b.nnz > 0)
                HIP_TRY(sp_launch(build_items_kernel, dgrid, st, (const int32_t *)cp, (const int64_t *)ic, (int)d, seg, b.e0, dptr<SpItem>(b.items_buf),
                                  dptr<SpLong>(b.longs_buf), dptr<int32_t>(seen)));
            core->max_runs = std::max(core->max_runs, b.n_runs);
        }
        // the columns with an entry: the one array of d elements that the host keeps (ppca_sparse_empty_dimensions does no device work)
        std::vector<int32_t> sh((size_t)d);
        HIP_TRY(hipMemcpyAsync(sh.data(), seen->p, sizeof(int32_t) * (size_t)d, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int32_t j = 0; j < d; ++j) core->empty[(size_t)j] = sh[(size_t)j] ? 0 : 1;
    }
    core->build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out = core;
    return PPCA_OK;
}

// the split of sp's entries into two cores; T: the integer of the scanned flags
template <class T>
int sb_split(ppca_ctx *ctx, const ppca_sparse *sp, double lo, double hi, uint64_t seed, int64_t row_offset, std::shared_ptr<SpCore> *train,
             std::shared_ptr<SpCore> *held, int64_t *counts_out) {
    const SpCore &c = *sp->core;
    hipStream_t st = ctx->stream;
    const int64_t n = c.n, nnz = c.nnz;
    BufRef at, scan, tp, hp, tc, hc, tv, hv;
    if (int rc = sb_alloc(sizeof(T) * (size_t)(nnz + 1), &at)) return rc;
    if (int rc = sb_alloc(sizeof(T) * (size_t)sb_scan_scratch(nnz), &scan)) return rc;
    if (nnz > 0)
        HIP_TRY(sp_launch(split_flag_kernel<T>, sp_elementwise_grid(nnz, ctx->n_cu), st, c.row_ptr(), c.col(), n, nnz, lo, hi, seed, row_offset,
                          dptr<T>(at)));
    if (int rc = sb_scan(ctx, dptr<T>(at), nnz, dptr<T>(scan))) return rc;
    T nheld = 0;
    HIP_TRY(hipMemcpyAsync(&nheld, dptr<T>(at) + nnz, sizeof(T), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t nh = (int64_t)nheld, nt = nnz - nh;
    if (int rc = sb_alloc(sizeof(int64_t) * (size_t)(n + 1), &tp)) return rc;
    if (int rc = sb_alloc(sizeof(int64_t) * (size_t)(n + 1), &hp)) return rc;
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)nt, &tc)) return rc;
    if (int rc = sb_alloc(sizeof(int32_t) * (size_t)nh, &hc)) return rc;
    if (int rc = sb_alloc(sizeof(double) * (size_t)nt, &tv)) return rc;
    if (int rc = sb_alloc(sizeof(double) * (size_t)nh, &hv)) return rc;
    if (nnz > 0)
        HIP_TRY(sp_launch(split_compact_kernel<T>, sp_elementwise_grid(nnz, ctx->n_cu), st, c.col(), sp->val(), nnz, (const T *)dptr<T>(at),
                          dptr<int32_t>(tc), dptr<double>(tv), dptr<int32_t>(hc), dptr<double>(hv)));
    HIP_TRY(sp_launch(split_rowptr_kernel<T>, sp_elementwise_grid(n + 1, ctx->n_cu), st, c.row_ptr(), n, (const T *)dptr<T>(at), dptr<int64_t>(tp),
                      dptr<int64_t>(hp)));
    at.reset();
    scan.reset();
    if (int rc = sb_build_core(ctx, n, c.d, tp, tc, tv, c.block_rows, c.segment, 0, train)) return rc;
    if (int rc = sb_build_core(ctx, n, c.d, hp, hc, hv, c.block_rows, c.segment, 0, held)) return rc;
    if (counts_out) {
        counts_out[0] = nt;
        counts_out[1] = nh;
    }
    return PPCA_OK;
}

}  // namespace

// ------------------------------------------------------------------ C-ABI
extern "C" int ppca_from_device_sparse(int64_t n, int32_t d, ppca_ctx *ctx, const int64_t *row_ptr_dev, const int32_t *col_dev,
                                       const double *val_dev, const double *weights_dev, int64_t block_rows, int32_t segment, ppca_sparse **out) {
    if (!ctx || !out) return fail(PPCA_ERR_INVALID, "null argument");
    if (n < 0 || d < 1 || !row_ptr_dev) return fail(PPCA_ERR_INVALID, "bad shape or null row_ptr");
    if (block_rows < 0 || block_rows > INT32_MAX || segment < 0) return fail(PPCA_ERR_INVALID, "block_rows and segment must be >= 0");
    USE_CTX(ctx);
    auto sp = std::make_unique<ppca_sparse>();
    sp->ctx = ctx;
    if (int rc = sb_build_core(ctx, n, d, dev_borrow(row_ptr_dev), dev_borrow(col_dev), dev_borrow(val_dev), block_rows, segment, 1, &sp->core))
        return rc;
    if (weights_dev) {
        sp->wbuf = dev_borrow(weights_dev);
        sp->w = weights_dev;
    }
    *out = sp.release();
    return PPCA_OK;
}

extern "C" int ppca_n_blocks_sparse(int64_t *n_blocks_out, const ppca_sparse *sp) {
    if (!n_blocks_out || !sp) return fail(PPCA_ERR_INVALID, "null argument");
    *n_blocks_out = (int64_t)sp->core->blocks.size();
    return PPCA_OK;
}

extern "C" int ppca_index_to_host_sparse(int64_t block, ppca_sparse *sp, int64_t *counts_out, int64_t *col_ptr_out, int32_t *t_row_out,
                                         double *t_val_out, int32_t *rowlist_out, void *items_out, void *longs_out) {
    if (!sp) return fail(PPCA_ERR_INVALID, "null argument");
    const SpCore &c = *sp->core;
    if (block == -1) {  // the container's own fields
        if (col_ptr_out || t_row_out || t_val_out || rowlist_out || items_out || longs_out)
            return fail(PPCA_ERR_INVALID, "block -1 has counts alone");
        if (counts_out) {
            const int64_t v[13] = {c.n, c.nnz, c.block_rows, c.segment, c.max_rows, c.max_runs, c.nonempty_rows, c.d, (int64_t)c.blocks.size(),
                                   0, 0, 0, 0};
            std::copy(v, v + 13, counts_out);
        }
        return PPCA_OK;
    }
    if (block < 0 || block >= (int64_t)c.blocks.size())
        return fail(PPCA_ERR_INVALID, "block %lld is outside [0, %lld)", (long long)block, (long long)c.blocks.size());
    const SpBlock &b = c.blocks[(size_t)block];
    ppca_ctx *ctx = sp->ctx;
    USE_CTX(ctx);
    hipStream_t st = ctx->stream;
    if (counts_out) {
        const int64_t v[13] = {b.row0, b.rows, b.e0, b.nnz, b.nbin[0], b.nbin[1], b.nbin[2], b.bin_off[0], b.bin_off[1], b.bin_off[2],
                               b.n_items, b.n_long, b.n_runs};
        std::copy(v, v + 13, counts_out);
    }
    std::vector<SpItem> items;
    if (col_ptr_out) items.resize((size_t)b.n_items);
    SpItem *ih = col_ptr_out ? items.data() : static_cast<SpItem *>(items_out);
    if (ih && b.n_items) HIP_TRY(hipMemcpyAsync(ih, b.items(), sizeof(SpItem) * (size_t)b.n_items, hipMemcpyDeviceToHost, st));
    if (longs_out && b.n_long) HIP_TRY(hipMemcpyAsync(longs_out, b.longs(), sizeof(SpLong) * (size_t)b.n_long, hipMemcpyDeviceToHost, st));
    if (t_row_out && b.nnz) HIP_TRY(hipMemcpyAsync(t_row_out, c.trow() + b.e0, sizeof(int32_t) * (size_t)b.nnz, hipMemcpyDeviceToHost, st));
    if (t_val_out && b.nnz) HIP_TRY(hipMemcpyAsync(t_val_out, sp->tval() + b.e0, sizeof(double) * (size_t)b.nnz, hipMemcpyDeviceToHost, st));
    if (rowlist_out && b.rows) HIP_TRY(hipMemcpyAsync(rowlist_out, b.rowlist(), sizeof(int32_t) * (size_t)b.rows, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (col_ptr_out) {  // recomputed from the items: a column's entries are the sum of its items' lengths
        std::fill(col_ptr_out, col_ptr_out + c.d + 1, (int64_t)0);
        for (const SpItem &it : items) col_ptr_out[it.col + 1] += it.len;
        for (int32_t j = 0; j < c.d; ++j) col_ptr_out[j + 1] += col_ptr_out[j];
        if (items_out && b.n_items) std::memcpy(items_out, items.data(), sizeof(SpItem) * items.size());
    }
    return PPCA_OK;
}

extern "C" int ppca_heldout_split_sparse(double lo, double hi, uint64_t seed, int64_t row_offset, ppca_ctx *ctx, ppca_sparse *sp,
                                         ppca_sparse **train_out, ppca_sparse **held_out, int64_t *counts_out) {
    if (!ctx || !sp || !train_out || !held_out) return fail(PPCA_ERR_INVALID, "null argument");
    if (!(lo >= 0.0 && lo <= hi && hi <= 1.0)) return fail(PPCA_ERR_INVALID, "the range must satisfy 0 <= lo <= hi <= 1");
    if (row_offset < 0) return fail(PPCA_ERR_INVALID, "row_offset must be >= 0");
    if (sp->ctx->device != ctx->device) return fail(PPCA_ERR_INVALID, "dataset and context live on different devices");
    USE_CTX(ctx);
    auto train = std::make_unique<ppca_sparse>(), held = std::make_unique<ppca_sparse>();
    const int rc = sp->core->nnz <= INT32_MAX ? sb_split<int32_t>(ctx, sp, lo, hi, seed, row_offset, &train->core, &held->core, counts_out)
                                              : sb_split<int64_t>(ctx, sp, lo, hi, seed, row_offset, &train->core, &held->core, counts_out);
    if (rc) return rc;
    for (ppca_sparse *part : {train.get(), held.get()}) {  // the parent's weights, shared
        part->ctx = ctx;
        part->wbuf = sp->wbuf;
        part->w = sp->w;
    }
    *train_out = train.release();
    *held_out = held.release();
    return PPCA_OK;
}
