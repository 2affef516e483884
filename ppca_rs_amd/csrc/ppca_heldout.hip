// ppca_heldout.hip -- scoring a model on held-out entries (ppca_dataset_holdout, ppca_heldout_score).
//
//   holdout_kernel   one sweep over an N x d dataset (row stride ldx): one read, two writes.  Entry (i, j) of global row
//                    g = row_offset + i draws u = (row_word(row_key(seed, 8, g), j) >> 11) 2^-53 from the counter-based generator of
//                    ppca_sweep.hpp (u01_floor, STREAM_HOLDOUT); an observed (finite) entry is HELD iff lo <= u < hi (a fraction f is
//                    the range [0, f); the K folds are the ranges between neighbouring edges f / K):
//                      held:   train = NaN, held = x (the bits as they are)        kept:   train = x, held = NaN
//                      masked (any non-finite value): NaN in both
//                    part[workgroup][2] = the workgroup's [kept, held] entry counts (integers, as doubles).  Nothing depends on the
//                    grid.  The layout is scale_kernel's: a thread owns a 16-byte column pair (one column when d is odd or a row is not
//                    16-byte aligned) of HOLD_ROWS rows per step, loads and stores are non-temporal, a workgroup takes one contiguous
//                    run of rows.
//   heldout_score_kernel   for every finite entry x of `held` in a row whose posterior given `train` is (z, Sigma):
//                      m = mean_j + c_j^T z,  v = sigma^2 + c_j^T Sigma c_j,  e = x - m,  l = -1/2 (ln 2 pi + ln v + e^2 / v)
//                    One wave per row (grid-stride).  The row of `held` is read 64 columns at a time; the finite entries of a block are
//                    found by ballot and appended (column, value) to a list in LDS, and whenever the list holds 64 entries -- and at the
//                    end of the row -- one lane per LISTED entry does the k^2 multiply-adds of c_j^T Sigma c_j (Sigma and z of the row
//                    in LDS, the inner loop of loo_kernel), so that the work follows the number of held entries, not d.  l_j goes
//                    to its column's slot of an LDS row (0 elsewhere) and the row's sum is taken over the columns in an order that
//                    depends on d alone: lane t adds columns t, t + 64, ..., then a 64-lane butterfly.  Column sums [w | w l | w e^2 |
//                    w e^2 / v] and [entries | rows with an entry] accumulate in LDS over the workgroup's rows in row order (a column is
//                    listed once per row, one lane owns it: no atomics) and leave as part[workgroup][4 d + 2].  The mixture runs the
//                    same kernel once per component in a form that folds (m, v, l) into per-entry state, then a form that sums it.
//                    Two further density arms of the one-model form, for k <= 16 and d <= 1024:
//                      known precisions   the wave also reads the row of the held precisions q; an entry is listed iff x is finite
//                                         and q is finite and > 0, with q as the list's third array; v = sigma^2 / q + c_j^T Sigma c_j.
//                                         A q < 0 or +inf at a finite x is counted (part[4 d + 2]) and not listed.
//                      Student-t          a prologue reads the row of `train` 64 columns at a time: m = its finite entries (ballot),
//                                         |r|^2 = sum (x - mean_j - c_j^T z)^2 with the z in LDS (per lane in column order, then a
//                                         butterfly), delta = (|r|^2 + sigma^2 |z|^2) / sigma^2.  With nu_m = nu + m:
//                                         s = (sigma^2 + c_j^T Sigma c_j) (nu + delta) / nu_m,
//                                         l = tbl[m] - 1/2 ln s - 1/2 (nu_m + 1) log1p(e^2 / (nu_m s)), and the z^2 sum takes
//                                         e^2 / (s nu_m / (nu_m - 2)), 0 when nu_m <= 2 (no variance).
#include <algorithm>

#include "ppca_sweep.hpp"

namespace ppca {
namespace {

constexpr int HOLD_THREADS = 256;
constexpr int HOLD_ROWS = 4;  // row steps a thread has in flight

struct HoldArgs {
    const double *X;
    int64_t ldx, n;
    int d;
    double lo, hi;  // held: lo <= u < hi
    uint64_t seed;
    int64_t row_offset;
    double *train, *held;  // n x d each (row stride d)
    double *part;          // [grid][2]: kept, held
    int tpr_log2;          // threads per row = 1 << tpr_log2
    int64_t rows_per_wg;
};

template <int VEC>
__global__ __launch_bounds__(HOLD_THREADS) void holdout_kernel(HoldArgs a) {
    __shared__ unsigned long long red[2][HOLD_THREADS / 64];
    const int t = threadIdx.x, d = a.d;
    int tpr, rps, tc, tr, slots;
    int64_t r0, r1;
    sweep_layout<HOLD_THREADS, VEC>(t, d, a.tpr_log2, a.rows_per_wg, a.n, tpr, rps, tc, tr, slots, r0, r1);
    const double qnan = __builtin_nan("");
    unsigned long long kept = 0, heldc = 0;
    for (int c0 = 0; c0 < slots; c0 += tpr) {
        const int slot = c0 + tc;
        const bool on = slot < slots;
        const int j = slot * VEC;
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rps * HOLD_ROWS) {
            Vec<VEC> x[HOLD_ROWS];
#pragma unroll
            for (int u = 0; u < HOLD_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                if (on && r < r1) {
                    x[u] = load_vec<VEC, true>(a.X + r * a.ldx + j);
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) x[u].v[v] = qnan;
                }
            }
#pragma unroll
            for (int u = 0; u < HOLD_ROWS; ++u) {
                const int64_t r = rb + (int64_t)u * rps + tr;
                if (!(on && r < r1)) continue;
                const uint64_t key = row_key(a.seed, STREAM_HOLDOUT, (uint64_t)(a.row_offset + r));
                Vec<VEC> tv, hv;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double xv = x[u].v[v];
                    const bool obs = __builtin_isfinite(xv);
                    const double uu = u01_floor(row_word(key, (uint64_t)(j + v)));
                    const bool hold = obs && uu >= a.lo && uu < a.hi;
                    tv.v[v] = (obs && !hold) ? xv : qnan;
                    hv.v[v] = hold ? xv : qnan;
                    kept += (obs && !hold) ? 1u : 0u;
                    heldc += hold ? 1u : 0u;
                }
                store_vec<VEC, true>(a.train + r * d + j, tv);
                store_vec<VEC, true>(a.held + r * d + j, hv);
            }
        }
    }
    // the workgroup's counts (integers: any order gives the same sum): a butterfly per wave, then the waves in index order
    for (int off = 32; off > 0; off >>= 1) {
        kept += __shfl_down(kept, off, 64);
        heldc += __shfl_down(heldc, off, 64);
    }
    if ((t & 63) == 0) {
        red[0][t >> 6] = kept;
        red[1][t >> 6] = heldc;
    }
    __syncthreads();
    if (t < 2) {
        unsigned long long s = 0;
        for (int w = 0; w < HOLD_THREADS / 64; ++w) s += red[t][w];
        a.part[(int64_t)blockIdx.x * 2 + t] = (double)s;
    }
}

// ---- the score
constexpr int HELD_LIST = 128;  // the list holds < 64 entries before a block of <= 64 is appended

struct HeldArgs {
    const double *H;       // the chunk's rows of `held`
    int64_t ldh;
    const double *w;       // nullable (= 1): the chunk's row weights (train's)
    int d, k;
    int64_t n_rows;
    const double *model;   // [sigma, sigma^2, ln sigma, 0 | C (d x k) | mean (d)]   (HELD_FINISH: unused)
    const double *states;  // n_rows x k                                                (HELD_FINISH: unused)
    const double *covs;    // n_rows x k x k                                            (HELD_FINISH: unused)
    double *per_row;       // nullable, n_rows
    double *part;          // [grid][heldout_part_len(d, k)]                            (HELD_FOLD: unused)
    int sums_in_lds;       // the row's l slots and the column sums live in LDS (else in the workgroup's own partial)
    // the mixture: the chunk's rows of the n x nm log posteriors, the component folded, and the per-entry state (n_rows x d each,
    // touched at the held entries only): running maximum mx and scaled sum sm of lp_c + l_c, A = sum a_c (m_c - x), V = sum a_c v_c,
    // Q = sum a_c (m_c - x)^2 with a_c = exp(lp_c)
    const double *logpost;
    int comp, nm, first;
    double *mx, *sm, *fa, *fv, *fq;
    // the family arms (HELD_MODEL only).  HELD_PREC: the chunk's rows of the held precisions.  HELD_T: the chunk's rows of `train`,
    // tbl[0 .. d] (ppca_t_pred_table_host) and the degrees of freedom
    const double *Q;
    int64_t ldq;
    const double *T;
    int64_t ldt;
    const double *tbl;
    double dof;
};

enum { HELD_MODEL = 0, HELD_FOLD = 1, HELD_FINISH = 2 };
enum { HELD_GAUSS = 0, HELD_PREC = 1, HELD_T = 2 };  // the density of a held entry (the mixture forms are Gaussian)

// MODE HELD_MODEL: the score of one model.  HELD_FOLD: the same per-entry (m, v, l) of mixture component a.comp, folded into the
// per-entry state instead of summed (the first component initialises it; a component of weight 0 contributes nothing).
// HELD_FINISH: per held entry l = mx + ln sm, e = -A, variance V + max(Q - A^2, 0) from the folded state (k = 0: no Sigma), summed as
// HELD_MODEL sums its own.
// LDS: Sigma padded to kq = pad16(k) columns with zeros (k x kq) | z padded (kq) | the list's values (HELD_LIST) | the list's
// columns (HELD_LIST ints) | when they fit 64 KiB with the rest (sums_in_lds): the column sums (4 d), l of the row's columns (d).
// Otherwise those 5 d doubles are the workgroup's own partial in global memory, [sums (4 d) | 2 counts | l slots (d, back at 0 when
// the kernel ends)], read and written by this wave alone with a barrier between a write and the next read of a slot.
// FAM (HELD_MODEL only) HELD_PREC: the list has a third array, the entries' precisions, behind its values, and the partial one more
// count, [sums (4 d) | 2 counts | bad precisions].  HELD_PREC and HELD_T cover k <= 16 and d <= 1024, where the sums always fit in
// LDS (under 46 KiB in all): their instantiations take that branch at compile time and the global-partial one does not exist in them.
template <int MODE, int FAM = HELD_GAUSS>
__global__ __launch_bounds__(64) void heldout_score_kernel(HeldArgs a) {
    static_assert(FAM == HELD_GAUSS || MODE == HELD_MODEL, "the family arms are forms of the one-model score");
    extern __shared__ double lds[];
    const int k = a.k, d = a.d, kq = pad16(k), lane = threadIdx.x;
    const bool in_lds = FAM != HELD_GAUSS ? true : a.sums_in_lds != 0;
    double *S = lds, *Z = S + (size_t)k * kq, *lx = Z + kq;
    double *lq = lx + HELD_LIST;  // (HELD_PREC)
    int *lj = reinterpret_cast<int *>(lx + (FAM == HELD_PREC ? 2 : 1) * HELD_LIST);
    double *part = nullptr, *cs = nullptr, *L = nullptr;
    double n_entries = 0.0, n_rows_held = 0.0, n_bad = 0.0;  // (lane 0's are the workgroup's)
    if constexpr (MODE != HELD_FOLD) {
        part = a.part + (int64_t)blockIdx.x * ((int64_t)(in_lds ? 4 : 5) * d + (FAM == HELD_PREC ? 3 : 2));
        cs = in_lds ? reinterpret_cast<double *>(lj) + HELD_LIST / 2 : part;
        L = in_lds ? cs + (size_t)4 * d : part + (size_t)4 * d + 2;
        for (int e = lane; e < 4 * d; e += 64) cs[e] = 0.0;
        for (int e = lane; e < d; e += 64) L[e] = 0.0;
        __syncthreads();
    }
    const double sig2 = MODE != HELD_FINISH ? a.model[1] : 0.0;
    const double *C = MODE != HELD_FINISH ? a.model + 4 : nullptr;
    const double *mu = MODE != HELD_FINISH ? C + (int64_t)d * k : nullptr;
    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        if constexpr (MODE != HELD_FINISH) {
            const double *Sg = a.covs + r * k * k;
            for (int e = lane; e < k * kq; e += 64) {
                const int ra = e / kq, cb = e % kq;
                S[e] = cb < k ? Sg[ra * k + cb] : 0.0;
            }
            for (int e = lane; e < kq; e += 64) Z[e] = e < k ? a.states[r * k + e] : 0.0;
        }
        const double wr = (MODE != HELD_FOLD && a.w) ? a.w[r] : 1.0;
        const double lp = MODE == HELD_FOLD ? a.logpost[r * a.nm + a.comp] : 0.0;
        const double *h = a.H + r * a.ldh;
        int cnt = 0, row_cnt = 0;  // (wave-uniform)
        __syncthreads();
        double t_num = 0.0, t_scale = 1.0, t_norm = 0.0;  // HELD_T (wave-uniform): nu_m, (nu + delta) / nu_m, tbl[m]
        if constexpr (FAM == HELD_T) {
            const double *tr = a.T + r * a.ldt;
            int m = 0;
            double rr = 0.0;
            for (int j0 = 0; j0 < d; j0 += 64) {
                const int j = j0 + lane;
                const double xv = j < d ? __builtin_nontemporal_load(tr + j) : __builtin_nan("");
                const bool fin = __builtin_isfinite(xv);
                m += __popcll(__ballot(fin));
                if (fin) {
                    const double *cj = C + (int64_t)j * k;
                    double dot = 0.0;
                    for (int i = 0; i < k; ++i) dot = fma(cj[i], Z[i], dot);
                    const double res = (xv - mu[j]) - dot;
                    rr = fma(res, res, rr);
                }
            }
            for (int off = 32; off > 0; off >>= 1) rr += __shfl_xor(rr, off, 64);  // (the same sum on every lane)
            double zz = 0.0;
            for (int i = 0; i < k; ++i) zz = fma(Z[i], Z[i], zz);
            const double delta = fma(sig2, zz, rr) / sig2;
            t_num = a.dof + (double)m;
            t_scale = (a.dof + delta) / t_num;
            t_norm = a.tbl[m];
        }
        for (int j0 = 0; j0 < d || cnt > 0; j0 += 64) {
            if (j0 < d) {
                const int j = j0 + lane;
                const double xv = j < d ? __builtin_nontemporal_load(h + j) : __builtin_nan("");
                bool fin = __builtin_isfinite(xv);
                double qv = 1.0;
                if constexpr (FAM == HELD_PREC) {
                    qv = j < d ? __builtin_nontemporal_load(a.Q + r * a.ldq + j) : 0.0;
                    n_bad += (double)__popcll(__ballot(fin && (qv < 0.0 || qv == __builtin_inf())));
                    fin = fin && qv > 0.0 && qv < __builtin_inf();  // (NaN or 0: not observed)
                }
                const unsigned long long bal = __ballot(fin);
                if (fin) {
                    const int at = cnt + __popcll(bal & ((1ull << lane) - 1ull));
                    lx[at] = xv;
                    lj[at] = j;
                    if constexpr (FAM == HELD_PREC) lq[at] = qv;
                }
                cnt += __popcll(bal);
                row_cnt += __popcll(bal);
                __syncthreads();
                if (cnt < 64 && j0 + 64 < d) continue;  // (uniform) not a full wave of entries yet, and more of the row to come
            }
            // lanes 0 .. min(cnt, 64) take one listed entry each
            const int take = cnt < 64 ? cnt : 64;
            if (lane < take) {
                const int j = lj[lane];
                const double xv = lx[lane];
                const int64_t o = r * d + j;
                double e2, v, l;
                if constexpr (MODE != HELD_FINISH) {
                    const double *cj = C + (int64_t)j * k;
                    // q = c_j^T Sigma c_j by blocks of 16 columns of Sigma: the loop of loo_kernel (ppca_loo.hip, see the note there)
                    // without |c_j|^2; the padding columns are 0
                    double dot = 0.0, q = 0.0;
                    for (int b0 = 0; b0 < k; b0 += 16) {
                        double acc[16];
#pragma unroll
                        for (int b = 0; b < 16; ++b) acc[b] = 0.0;
                        for (int i = 0; i < k; ++i) {
                            const double ci = cj[i];
                            if (b0 == 0) dot = fma(ci, Z[i], dot);
                            const double *Si = S + (size_t)i * kq + b0;
#pragma unroll
                            for (int b = 0; b < 16; ++b) acc[b] = fma(ci, Si[b], acc[b]);
                        }
#pragma unroll
                        for (int b = 0; b < 16; ++b)
                            if (b0 + b < k) q = fma(acc[b], cj[b0 + b], q);
                    }
                    const double m = mu[j] + dot, e = xv - m;
                    e2 = __dmul_rn(e, e);
                    if constexpr (FAM == HELD_T) {
                        v = (sig2 + q) * t_scale;  // the scale s of the predictive t
                        l = t_norm - 0.5 * log(v) - 0.5 * (t_num + 1.0) * log1p(e2 / (t_num * v));
                    } else {
                        v = (FAM == HELD_PREC ? sig2 / lq[lane] : sig2) + q;
                        l = -0.5 * (LOG_2PI + log(v) + e2 / v);
                    }
                    if constexpr (MODE == HELD_FOLD) {
                        double M = a.first ? -INFINITY : a.mx[o], Sm = a.first ? 0.0 : a.sm[o];
                        double A = a.first ? 0.0 : a.fa[o], V = a.first ? 0.0 : a.fv[o], Q = a.first ? 0.0 : a.fq[o];
                        const double tc = lp + l;
                        if (tc > M) {  // the log-sum-exp push of mix_loo_fold_kernel (ppca_loo.hip), which also rescales its W
                            Sm = Sm * exp(M - tc) + 1.0;
                            M = tc;
                        } else if (tc > -INFINITY) {
                            Sm += exp(tc - M);
                        }
                        const double ac = exp(lp);
                        if (ac > 0.0) {
                            A = fma(ac, -e, A);
                            V = fma(ac, v, V);
                            Q = fma(ac, e2, Q);
                        }
                        a.mx[o] = M;
                        a.sm[o] = Sm;
                        a.fa[o] = A;
                        a.fv[o] = V;
                        a.fq[o] = Q;
                    }
                } else {
                    const double A = a.fa[o];
                    e2 = __dmul_rn(A, A);
                    const double spread = __dsub_rn(a.fq[o], e2);  // (no contraction: exactly 0 for one component)
                    v = a.fv[o] + (spread > 0.0 ? spread : 0.0);
                    l = a.mx[o] + log(a.sm[o]);
                }
                if constexpr (MODE != HELD_FOLD) {
                    // (HELD_T: over the variance s nu_m / (nu_m - 2); none when nu_m <= 2, and the entry adds 0)
                    const double z2 = FAM == HELD_T ? (t_num > 2.0 ? e2 / (v * (t_num / (t_num - 2.0))) : 0.0) : e2 / v;
                    L[j] = l;
                    cs[j] += wr;
                    cs[d + j] = fma(wr, l, cs[d + j]);
                    cs[2 * d + j] = fma(wr, e2, cs[2 * d + j]);
                    cs[3 * d + j] = fma(wr, z2, cs[3 * d + j]);
                }
            }
            __syncthreads();
            // what is left of the list moves to its front
            const int rest = cnt - take;
            double mvx = 0.0, mvq = 0.0;
            int mvj = 0;
            if (lane < rest) {
                mvx = lx[take + lane];
                mvj = lj[take + lane];
                if constexpr (FAM == HELD_PREC) mvq = lq[take + lane];
            }
            __syncthreads();
            if (lane < rest) {
                lx[lane] = mvx;
                lj[lane] = mvj;
                if constexpr (FAM == HELD_PREC) lq[lane] = mvq;
            }
            cnt = rest;
            __syncthreads();
        }
        if constexpr (MODE != HELD_FOLD) {
            // the row's sum over its columns in index order per lane, then the butterfly; the slots go back to 0
            double lsum = 0.0;
            for (int j = lane; j < d; j += 64) {
                lsum += L[j];
                L[j] = 0.0;
            }
            for (int off = 32; off > 0; off >>= 1) lsum += __shfl_down(lsum, off, 64);
            if (lane == 0) {
                if (a.per_row) a.per_row[r] = lsum;
                n_entries += (double)row_cnt;
                n_rows_held += row_cnt > 0 ? 1.0 : 0.0;
            }
        }
        __syncthreads();  // S, Z and L are the next row's
    }
    if constexpr (MODE != HELD_FOLD) {
        if (in_lds)
            for (int e = lane; e < 4 * d; e += 64) part[e] = cs[e];
        if (lane == 0) {
            part[4 * d] = n_entries;
            part[4 * d + 1] = n_rows_held;
            if constexpr (FAM == HELD_PREC) part[4 * d + 2] = n_bad;
        }
    }
}

}  // namespace

int holdout_grid(int64_t n, int d, int n_cu) { return scale_grid(n, d, n_cu); }

hipError_t launch_holdout(const double *X, int64_t ldx, int64_t n, int d, double lo, double hi, uint64_t seed, int64_t row_offset,
                          double *train, double *held, double *part, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    const SweepCut cut = sweep_cut(d, ldx % 2 == 0, {X, train, held});
    HoldArgs a{X, ldx, n, d, lo, hi, seed, row_offset, train, held, part, cut.tpr_log2, (n + grid - 1) / grid};
    if (cut.vec)
        hipLaunchKernelGGL(holdout_kernel<2>, dim3((unsigned)grid), dim3(HOLD_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(holdout_kernel<1>, dim3((unsigned)grid), dim3(HOLD_THREADS), 0, s, a);
    return hipGetLastError();
}

static size_t held_lds_base(int k, int lists = 1) {  // lists: the list's arrays of doubles (values; HELD_PREC: and precisions)
    const int kq = pad16(k);
    return sizeof(double) * ((size_t)k * kq + kq + (size_t)lists * HELD_LIST) + sizeof(int) * HELD_LIST;
}
static bool held_sums_in_lds(int d, int k) { return held_lds_base(k) + sizeof(double) * (size_t)5 * d <= 64 * 1024; }
size_t heldout_score_lds_bytes(int d, int k) { return held_lds_base(k) + (held_sums_in_lds(d, k) ? sizeof(double) * (size_t)5 * d : 0); }
int64_t heldout_part_len(int d, int k) { return (int64_t)(held_sums_in_lds(d, k) ? 4 : 5) * d + 2; }

// Workgroups (one wave each): 16 per CU, fewer where the partials (grid x heldout_part_len doubles) would pass 64 MiB, never fewer
// than one per CU.
int heldout_score_grid(int64_t n_rows, int d, int k, int n_cu) {
    if (n_rows <= 0) return 0;
    const int64_t cu = std::max(n_cu, 1);
    const int64_t cap = ((int64_t)64 << 20) / ((int64_t)sizeof(double) * heldout_part_len(d, k));
    return (int)std::min<int64_t>(n_rows, std::max<int64_t>(cu, std::min<int64_t>(cu * 16, cap)));
}

template <int MODE, int FAM = HELD_GAUSS>
static hipError_t launch_held(const HeldArgs &a, size_t lds, int grid, hipStream_t s) {
    if (hipError_t e = lds > 64 * 1024 ? ensure_dynamic_lds<heldout_score_kernel<MODE, FAM>>(lds) : hipSuccess; e != hipSuccess) return e;
    hipLaunchKernelGGL((heldout_score_kernel<MODE, FAM>), dim3((unsigned)grid), dim3(64), lds, s, a);
    return hipGetLastError();
}

// The family arms: k <= 16 and d <= 1024 (the callers' checks), so the column sums and the l slots are in LDS.
bool heldout_family_covers(int d, int k) { return k >= 1 && k <= 16 && d >= 1 && d <= 1024; }
int64_t heldout_family_part_len(int d, bool prec) { return (int64_t)4 * d + (prec ? 3 : 2); }
int heldout_family_grid(int64_t n_rows, int n_cu) {
    return n_rows <= 0 ? 0 : (int)std::min<int64_t>(n_rows, (int64_t)std::max(n_cu, 1) * 16);
}

hipError_t launch_heldout_score_prec(const double *H, int64_t ldh, const double *Q, int64_t ldq, const double *w, int d, int k,
                                     int64_t n_rows, const double *model, const double *states, const double *covs, double *per_row,
                                     double *part, int grid, hipStream_t s) {
    if (n_rows <= 0 || grid <= 0) return hipSuccess;
    if (!heldout_family_covers(d, k)) return hipErrorInvalidValue;
    HeldArgs a{};
    a.H = H, a.ldh = ldh, a.Q = Q, a.ldq = ldq, a.w = w, a.d = d, a.k = k, a.n_rows = n_rows, a.model = model, a.states = states;
    a.covs = covs, a.per_row = per_row, a.part = part, a.sums_in_lds = 1;
    return launch_held<HELD_MODEL, HELD_PREC>(a, held_lds_base(k, 2) + sizeof(double) * (size_t)5 * d, grid, s);
}

hipError_t launch_heldout_score_t(const double *H, int64_t ldh, const double *T, int64_t ldt, const double *w, int d, int k,
                                  int64_t n_rows, const double *model, const double *states, const double *covs, const double *tbl,
                                  double dof, double *per_row, double *part, int grid, hipStream_t s) {
    if (n_rows <= 0 || grid <= 0) return hipSuccess;
    if (!heldout_family_covers(d, k)) return hipErrorInvalidValue;
    HeldArgs a{};
    a.H = H, a.ldh = ldh, a.T = T, a.ldt = ldt, a.w = w, a.d = d, a.k = k, a.n_rows = n_rows, a.model = model, a.states = states;
    a.covs = covs, a.tbl = tbl, a.dof = dof, a.per_row = per_row, a.part = part, a.sums_in_lds = 1;
    return launch_held<HELD_MODEL, HELD_T>(a, held_lds_base(k) + sizeof(double) * (size_t)5 * d, grid, s);
}

hipError_t launch_heldout_score(const double *H, int64_t ldh, const double *w, int d, int k, int64_t n_rows, const double *model,
                                const double *states, const double *covs, double *per_row, double *part, int grid, hipStream_t s) {
    if (n_rows <= 0 || grid <= 0) return hipSuccess;
    HeldArgs a{};
    a.H = H, a.ldh = ldh, a.w = w, a.d = d, a.k = k, a.n_rows = n_rows, a.model = model, a.states = states, a.covs = covs;
    a.per_row = per_row, a.part = part, a.sums_in_lds = held_sums_in_lds(d, k) ? 1 : 0;
    return launch_held<HELD_MODEL>(a, heldout_score_lds_bytes(d, k), grid, s);
}

hipError_t launch_heldout_fold(const double *H, int64_t ldh, int d, int k, int64_t n_rows, const double *model, const double *states,
                               const double *covs, const double *logpost, int comp, int nm, double *fold, int grid, hipStream_t s) {
    if (n_rows <= 0 || grid <= 0) return hipSuccess;
    const int64_t nd = n_rows * d;
    HeldArgs a{};
    a.H = H, a.ldh = ldh, a.d = d, a.k = k, a.n_rows = n_rows, a.model = model, a.states = states, a.covs = covs;
    a.logpost = logpost, a.comp = comp, a.nm = nm, a.first = comp == 0;
    a.mx = fold, a.sm = fold + nd, a.fa = fold + 2 * nd, a.fv = fold + 3 * nd, a.fq = fold + 4 * nd;
    return launch_held<HELD_FOLD>(a, held_lds_base(k), grid, s);
}

hipError_t launch_heldout_finish(const double *H, int64_t ldh, const double *w, int d, int64_t n_rows, const double *fold,
                                 double *per_row, double *part, int grid, hipStream_t s) {
    if (n_rows <= 0 || grid <= 0) return hipSuccess;
    const int64_t nd = n_rows * d;
    double *f = const_cast<double *>(fold);
    HeldArgs a{};
    a.H = H, a.ldh = ldh, a.w = w, a.d = d, a.k = 0, a.n_rows = n_rows, a.per_row = per_row, a.part = part;
    a.sums_in_lds = held_sums_in_lds(d, 0) ? 1 : 0;
    a.mx = f, a.sm = f + nd, a.fa = f + 2 * nd, a.fv = f + 3 * nd, a.fq = f + 4 * nd;
    return launch_held<HELD_FINISH>(a, heldout_score_lds_bytes(d, 0), grid, s);
}

}  // namespace ppca
