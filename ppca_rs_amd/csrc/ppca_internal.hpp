// ppca_internal.hpp -- declarations shared by the kernel units (ppca_*.hip: every launcher that
// crosses files is a host function declared here) and the C-ABI host layer (ppca_capi.hip).
// Not installed; the public surface is include/ppca_hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>

#include "../../include/ppca_hip.h"
#include "ppca_small.hpp"

namespace ppca {

// Device model buffer: [sigma, sigma^2, ln sigma, 0 | C (d x k row-major) | mean (d)]
constexpr int MODEL_HDR = 4;
inline int64_t model_len(int d, int k) { return MODEL_HDR + (int64_t)d * k + d; }

constexpr int FUSED_MAX_D = 256;  // one LDS-resident tile of 32 samples x 256 dims
constexpr int FUSED_MAX_K = 10;   // k(k+1)/2 + k + 1 <= 80 accumulator columns
constexpr int FUSED_TILE = 32;    // samples per tile
constexpr int FUSED_THREADS = 256;

struct PassArgs {
    const double *X;      // n x d row-major, non-finite = masked
    int64_t ldx;          // row stride in elements
    const double *w;      // n weights or nullptr (= 1)
    const int *rows;      // EM mode, nullable: gathered pass -- sample i is physical row rows[i] of X (w is indexed by i)
    int64_t n;
    const int *n_dev;     // nullable: the number of samples is read from device memory instead of n (gathered passes whose
                          // row count was produced on the device: no host round trip); the grid is sized for an upper bound
    int d;
    const double *model;  // device model buffer
    // EM mode
    double *part;         // [grid][stats_len] per-workgroup partial statistics
    // post mode (all nullable)
    double *scal_part;    // [grid][8] per-workgroup scalars (llk, sumw, ...)
    double *llks;         // n
    double *states;       // n x k
    double *covs;         // n x k x k
    double *recon;        // n x d
    int recon_mode;       // 0 smooth, 1 extrapolate, 2 smoothed cov diag, 3 extrapolated cov diag
    signed char *qtab;    // int8 Gram slice table of the current model (written by the launcher's qprep)
    double *qscale;       // its 64 dequantisation multipliers
    int *qflag;           // per column tile: 1 = the int8 form is not safe for this model (qprep's dynamic-range
                          // guard) -> the fp64-Gram instantiation runs; nullptr = run unconditionally
    int no_llk;           // EM mode: the caller does not read SC_LLK (mixture component steps): skip the
                          // per-sample logarithm of the weighted path
    double *dbg;          // diagnostic builds (-DPPCA_PHASE_TIMING): [grid][4] phase cycle sums
    // EM mode, the guard of the int8 form of the mask-side statistics (launch_em_wguard):
    double *errb;         // [grid][W_GUARD_NCOL]: per workgroup and column of [wP | wz | w], a bound of the rounding the fixed-point
                          // cut added to any sum of that column (written by em9_kernel; nullptr: not collected)
    const double *cpb;    // C as the A operands of em9_kernel's b = X~ C on v_mfma_f64_4x4x4, in operand order (CPB_DOUBLES, written
                          // by qprep_kernel: see cpb_index)
    const int *runflag;   // nullable: second stage of a guarded EM pass (launch_em_fallback): the fp64 instantiation of pass_kernel
                          // reads the verdict of reduce_wguard_kernel: 0 = return at once; 1 = the whole pass again; 2 = only the
                          // slices (runs of tiles, as the guarded launch dealt them) of the flagged workgroups `who`, each slice
                          // split over gridDim.x / n_flagged workgroups; nullptr: qflag decides as before
    const int *who;       // [n_flagged] (runflag[QF_NFLAGGED - QF_MODE]) ascending workgroup indices of the guarded launch
    int heavy_max;        // em9_kernel's back role: a tile with at most this many rows that do not fit the fixed-point form of the
                          // mask-side statistics sends those rows round it (exact fp64 adds) instead of raising its exponents; 0: every
                          // such tile raises them (rounds 3-5: ppca_ctx_set_heavy_rows, a test hook)
    int skip_qprep;       // the slice table / guard flags / operand-ordered C behind qtab are already those of `model` (written by
                          // finalize_qprep_kernel at the end of the previous EM step): the pass launches no qprep_kernel
};
// Guard words behind PassArgs::qflag (ints): [0, 8) the Gram guard's per-tile flags (qprep_kernel); [8] the fallback's mode (see
// PassArgs::runflag); [9] the verdict of the W-side check; [10] ticket counter of reduce_wguard_kernel's last-block election;
// [11] workgroups whose slices the fallback recomputes; [12] rows in those slices; [13] the Gram guard's verdict for the pass (the tile
// flags themselves are overwritten by the NEXT model's when the step's finalisation builds its table).
constexpr int QF_MODE = 8, QF_WVERDICT = 9, QF_TICKET = 10, QF_NFLAGGED = 11, QF_NROWS2 = 12, QF_GVERDICT = 13;
// What reduce_wguard_kernel needs beside the partials.
struct GuardArgs {
    const double *errb;   // [grid][W_GUARD_NCOL] rounding bounds of the workgroups' cuts; nullptr: no W-side check (kernels that
                          // do not cut their rows: only the Gram flags decide)
    double *es;           // [W_GUARD_NCOL] scratch: their column sums (written by the reduction's extra workgroups)
    int *qflag;           // the guard words above
    int *wgflag;          // [grid]: 1 = the workgroup's partial is replaced by the fallback's
    int *who;             // [grid]: the flagged workgroups, ascending (PassArgs::who of the fallback)
    int64_t n;            // the guarded pass's row count (n_dev nullable: read from the device)
    const int *n_dev;
    int d;
    int grid;             // workgroups of the guarded launch (= partials)
};
// Multi-component launches of the mixture step (round 6): the per-component pointers travel BY VALUE in the kernel arguments, so a
// launch covers at most MIX_MAX components (larger mixtures, or components of different state sizes, run component by component).
constexpr int MIX_MAX = 16;
struct MixLlkArgs {  // mix_llk8_kernel (ppca_llk.hip): the llk sweeps of all components in one launch
    const double *X;
    int64_t ldx, n;
    int d, nm;
    int runs_per_xcd;             // mix_llk_runs_per_xcd(grid, nm)
    const double *model[MIX_MAX];
    void *tab[MIX_MAX];           // the component's slice-table block (fused_qtab_view)
    double *llks[MIX_MAX];        // n per component
};
struct MixTabArgs {  // qprep_multi_kernel: slice tables + guard flags + operand-ordered C of nm models in one launch
    int d, nm;
    const double *model[MIX_MAX];
    void *tab[MIX_MAX];
};
struct MixFinalArgs {  // finalize_qprep_multi_kernel: the M-step finalisation of nm components + the new models' tables
    int d, nm;
    double tau;
    int has_ig;
    double alpha, beta;
    const double *stats[MIX_MAX];
    const double *min[MIX_MAX];
    double *mout[MIX_MAX];
    void *tab[MIX_MAX];
};
struct MixReduceArgs {  // reduce_wguard_multi_kernel: reduction + verdict of nm guarded EM passes in one launch
    int nm;
    int64_t len;
    const double *part[MIX_MAX];
    double *out[MIX_MAX];
    GuardArgs g[MIX_MAX];
};

// em9_kernel's b = X~ C on v_mfma_f64_4x4x4 (round 5): one instruction = four blocks = (two
// 4-dim groups kb) x (two 4-sample groups sb); its A operand is C^T: lane 16 k + 8 kb + 4 sb + i holds C[dim][4 c + i] with
// dim = 128 kq + 32 (q >> 2) + 16 kb + 4 (q & 3) + k for the wave's dimension half kq, step q = 0..15 and column group c -- the same
// value for sb = 0, 1, so a (kq, q, c) operand is 32 doubles, stored contiguously: entry (k, kb, i) at (2 k + kb) 4 + i.
constexpr int CPB_GROUPS = 3;  // column groups of 4 at k = FUSED_MAX_K = 10
constexpr int CPB_DOUBLES = 2 * 16 * CPB_GROUPS * 32;
constexpr int W_GUARD_NCOL = 80;  // 16 x ceil((k' + k + 1) / 16) at k = 10

// Raises hipFuncAttributeMaxDynamicSharedMemorySize of `Kernel` on the current device to at least `bytes`; a no-op when this device
// already has that much for this kernel.  The attribute is per device and per kernel: one table per kernel holds, per device, the
// largest size set so far (read without the lock by every launch; written under it, so that two callers with different sizes cannot
// leave the attribute below what the table says).  A device id beyond the table sets the attribute uncached.
template <auto Kernel>
hipError_t ensure_dynamic_lds(size_t bytes) {
    constexpr int TABLE = 64;
    static std::atomic<size_t> have[TABLE] = {};
    static std::mutex mu;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < TABLE;
    if (cached && have[dev].load(std::memory_order_acquire) >= bytes) return hipSuccess;
    std::lock_guard<std::mutex> lock(mu);
    if (cached && have[dev].load(std::memory_order_relaxed) >= bytes) return hipSuccess;
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        e != hipSuccess)
        return e;
    if (cached) have[dev].store(bytes, std::memory_order_release);
    return hipSuccess;
}

// Number of workgroups the fused pass wants for n rows on a device with n_cu CUs.
int fused_grid(int64_t n, int n_cu);
size_t fused_lds_bytes(int k);
size_t fused_qtab_bytes();  // device scratch the fused launchers need in PassArgs::qtab / qscale / qflag
void fused_qtab_layout(void *base, PassArgs &a);  // points the three at a buffer of fused_qtab_bytes()
// Runs only the slice-table / guard kernel of a model (what every fused pass launches first).  *forced = 0 / 1 when
// the environment pins the engine (int8 without guard / fp64), -1 when qflag decides.
hipError_t launch_gram_guard(int k, const PassArgs &a, hipStream_t s, int *forced);
// qprep_kernel itself, 1 <= k <= 16: the slice table, dequantisation multipliers and guard flags of `model` and, for k <= FUSED_MAX_K
// (where qscale must be the base of a fused_qtab_view block), the operand-ordered copy of C behind the table
hipError_t launch_qprep(int k, const double *model, int d, double *qscale, signed char *qtab, int *qflag, hipStream_t s);
int fused_gram_tiles(int k);  // number of qflag entries the guard writes for state size k
// Launchers.  Return hipSuccess or the launch error.
hipError_t launch_pass_em(int k, int grid, const PassArgs &a, hipStream_t s);
hipError_t launch_pass_post(int k, int grid, const PassArgs &a, hipStream_t s);
// The EM pass as an eight-wave workgroup, two roles (ppca_em9.hip): front waves stage / [G | b] / solve (pipelined across tiles) /
// cross, back waves contract the mask-side statistics on the int8 MFMA.  Honours a.qflag like the int8 instantiation of pass_kernel.
bool em9_covers(int k);
hipError_t launch_em9(int k, int grid, const PassArgs &a, hipStream_t s);
hipError_t em9_debug_counters(unsigned long long *out4, int reset, hipStream_t s);
// The EM pass for 11 <= k <= 16, d <= 256 as two fused kernels (ppca_em16.hip): E-step sweep over X writing the rows
// [wP | wz | w] and the tiles' sample masks, then the mask-side statistics on the int8 MFMA.  Both write disjoint parts of
// part[grid][stats_len] (reduce with launch_reduce_partials).
struct Em16Launch {
    const double *X;
    int64_t ldx;
    const double *w;       // nullable
    int64_t n;
    int d;
    const double *model;
    double *part;          // [grid][stats_len]
    signed char *qtab;     // int8 Gram slice table of the model, em16_qtab_bytes(k) (launch_qprep)
    double *qscale;        // 16 x tiles dequantisation multipliers
    int *qflag;            // [tiles] guard flags; any set -> the Gram rows are read from Gext
    const double *Gext;    // [n][k'] packed Gram rows of the fp64 engine (read only when the guard tripped)
    double *Wrows;         // [n][em16_ncol(k)] scratch: the rows handed from the first kernel to the second
    unsigned *Mb;          // [ceil(n / 32)][256] scratch: per tile and dimension, the 32 sample bits
    int no_llk;
    double *dbg;
};
// diagnostic counters of the int8 statistics contraction (see ppca_em9.hip): read (and optionally reset) on the current device
hipError_t em16_debug_counters(unsigned long long *out4, int reset, hipStream_t s);
bool em16_covers(int d, int k);
int em16_ncol(int k);
size_t em16_qtab_bytes(int k);
hipError_t launch_em16(int k, int grid, const Em16Launch &a, hipStream_t s);
// The log-likelihood sweep alone (ppca_llk.hip): per-sample llks (nullable) and the per-workgroup scalars; honours
// a.qflag like the int8 instantiation of pass_kernel.
hipError_t launch_llk8(int k, int grid, const PassArgs &a, hipStream_t s);
// PPCAModel::smooth / extrapolate (recon modes 0 / 1) on the same eight-wave sweep (ppca_llk.hip, llk8_run<K, OUT>)
bool recon8_covers(const PassArgs &a);
hipError_t launch_recon8(int k, int grid, const PassArgs &a, hipStream_t s);
// ... of ALL components of a mixture in one launch (same state size k <= FUSED_MAX_K, nm <= MIX_MAX): units = (component, run of
// tiles), dealt so that the workgroups of one XCD walk the same rows for the different components (X from HBM once per iteration)
int mix_llk_runs_per_xcd(int grid, int nm);
hipError_t launch_mix_llk8(int k, int grid, const MixLlkArgs &a, hipStream_t s);
// the fp64-Gram instantiation of the post pass alone, behind a.qflag (the fallback of the int8 llk sweeps: returns at once unless the
// model's table tripped the dynamic-range guard)
hipError_t launch_pass_post_fp64(int k, int grid, const PassArgs &a, hipStream_t s);
int fused_gram_mode();  // 0: int8 behind the guard (default); 1: fp64 pinned (PPCA_GRAM_FP64=1); 2: int8 without guard (tuning builds)
hipError_t launch_qprep_multi(int k, const MixTabArgs &a, hipStream_t s);
hipError_t launch_finalize_qprep_multi(int k, const MixFinalArgs &a, hipStream_t s);
hipError_t launch_reduce_wguard_multi(int k, const MixReduceArgs &a, hipStream_t s);
hipError_t launch_reduce_partials(const double *part, int grid_parts, int64_t len, double *out, hipStream_t s, int accumulate = 0,
                                  const int *run_if = nullptr);  // run_if: device flag; the kernel returns at once when it is 0
// A guarded EM pass of the fused path after launch_pass_em, in two launches (round 5; rounds 3-4: reduction, wguard_kernel,
// fp64 pass, second reduction):
//   launch_reduce_wguard   sums the partials into `stats` (the fixed order of launch_reduce_partials); the LAST workgroup of
//                          that reduction then decides on the device what the second stage does (GuardArgs, QF_MODE): nothing;
//                          the whole pass again on the fp64 engine (the model tripped the Gram guard, or too many workgroups are
//                          flagged); or only the slices of the workgroups whose cut dominates the rounding bound of a column whose
//                          reduced diagonal entry of S is not large against it -- an outlier row costs its workgroup's slice,
//                          spread over the whole grid, not the pass.
//   launch_em_fallback     the fp64 instantiation of the pass behind that mode (returns at once on 0) into `part2`, then
//                          stats = sum of the un-flagged workgroups' partials + sum of part2 (returns at once on 0).
// Both return hipSuccess without launching anything when the stage does not apply (an engine pinned by the environment,
// kernel-tuning builds): *applies_out tells.
hipError_t launch_reduce_wguard(int k, const double *part, int64_t len, double *stats, const GuardArgs &g, hipStream_t s, bool *applies_out);
hipError_t launch_em_fallback(int k, int grid, PassArgs a, const GuardArgs &g, const double *part, double *part2, int64_t len, double *stats,
                              hipStream_t s);
// its second half alone (what launch_em_fallback ends with: the pass is ppca_pass.hip's, the reduction ppca_kernels.hip's)
hipError_t launch_reduce_fallback(const double *part, const double *part2, const GuardArgs &g, int64_t len, double *stats, hipStream_t s);
// finalize_kernel + the slice table / guard flags / operand-ordered C of the NEW model in one launch (the plain EM step: the next pass of
// that model then runs with PassArgs::skip_qprep)
hipError_t launch_finalize_qprep(int k, int d, const double *stats, const double *model_in, double *model_out, double tau, int has_ig,
                                 double alpha, double beta, const PassArgs &tab, hipStream_t s);
hipError_t launch_finalize(int k, int d, const double *stats, const double *model_in, double *model_out, double tau,
                           int has_ig, double alpha, double beta, hipStream_t s);
hipError_t launch_synth(const double *c_dev, const double *mean_dev, double *z_work, double *x_out, int64_t row_offset,
                        int64_t n_rows, int d, int k, double sigma, double mask_prob, int mask_kind, int mask_run,
                        uint64_t seed, hipStream_t s);
hipError_t launch_column_presence(const double *X, int64_t ldx, int64_t n, int d, int *present, hipStream_t s);
hipError_t launch_fill(double *p, int64_t n, double v, hipStream_t s);
// dst[i] = finite(src[i]) ? src[i] : NaN (src, dst 16-byte aligned)
hipError_t launch_canon_copy(const double *src, double *dst, int64_t n, hipStream_t s);
hipError_t launch_scale_rows(double *X, int64_t ldx, int d, const int64_t *rows_dev, int64_t n_rows, double factor, hipStream_t s);
// debug: C/D layout probe of v_mfma_f64_16x16x4_f64 (out: 16 x 16 row-major)
hipError_t launch_mfma_i8_probe(const int *a, const int *b, int *out, hipStream_t s);
hipError_t launch_mfma_probe(const double *a16x4, const double *b4x16, double *out16x16, hipStream_t s);

// generic split pipeline (ppca_generic.hip): any d, k <= GENERIC_MAX_K (65..128: the same int8-sliced contractions, one sample per
// wave in the blocked solver, and a finalisation whose k x k row systems are what 160 KB of LDS hold)
// trace (nullable): the record of the pass's host-side decisions, overwritten (test hook: ppca_generic_last_trace)
constexpr int GENERIC_MAX_K = 128;
size_t generic_workspace_bytes(int d, int k, int64_t n);
hipError_t generic_em_accumulate(const double *X, int64_t ldx, const double *w, int64_t n, int d, int k,
                                 const double *model, double *stats, void *ws, int n_cu, hipStream_t s,
                                 ppca_generic_trace *trace);
hipError_t generic_post(const double *X, int64_t ldx, const double *w, int64_t n, int d, int k, const double *model,
                        double *scal8, double *llks, double *states, double *covs, double *recon, int recon_mode,
                        void *ws, int n_cu, hipStream_t s, ppca_generic_trace *trace);
hipError_t generic_gram_guard(int d, int k, const double *model, void *ws, hipStream_t s, const int **flag_dev, int *forced);
hipError_t generic_finalize(int k, int d, const double *stats, const double *model_in, double *model_out, double tau,
                            int has_ig, double alpha, double beta, int n_cu, hipStream_t s);

// posterior sampling (ppca_sample.hip): the draw of DESIGN.md section 4.7 for rows [row0, row0 + n_rows) of a dataset from their
// posterior means / covariances (states, covs: the chunk's own rows) into out (dataset rows x d); choice (nullable): only rows
// whose choice[row] == comp are written.  mix_choose: a component per row from the log posteriors (n x nm).
size_t posterior_draw_lds_bytes(int k);
hipError_t launch_posterior_draw(const double *X, int64_t ldx, int d, int k, int64_t n_rows, int64_t row0, int64_t row_offset,
                                 const double *model, const double *states, const double *covs, double *out, int mode,
                                 uint64_t seed, const int *choice, int comp, int n_cu, hipStream_t s);
hipError_t launch_mix_choose(const double *logpost, int64_t n, int nm, uint64_t seed, int64_t row_offset, int *choice,
                             hipStream_t s);

// leave-one-out predictive (ppca_loo.hip): for rows [0, n_rows) of a chunk with their posterior means / covariances
// (states, covs), the predictive of every entry given the row's other observed entries -- mean, var (nullable, n_rows x d), the
// per-entry log-densities ell (nullable, n_rows x d, 0 on masked entries) and their row sums llks (nullable, n_rows).
size_t loo_lds_bytes(int k);
hipError_t launch_loo(const double *X, int64_t ldx, int d, int k, int64_t n_rows, const double *model, const double *states,
                      const double *covs, double *mean, double *var, double *ell, double *llks, int n_cu, hipStream_t s);
// The mixture's combination over a chunk (logpost: the chunk's rows of the n x nm log posteriors): fold component c's mean m and ell
// into mx, sm, wm (wm nullable: no mean wanted); finish: L into mx on observed entries, the mean into mean (nullable, may alias wm),
// llks (nullable); var: the second sweep, var (+)= a_cj (v_cj + (m_cj - mean_j)^2).
hipError_t launch_mix_loo_fold(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                               const double *m, const double *ell, double *mx, double *sm, double *wm, int first, hipStream_t s);
hipError_t launch_mix_loo_finish(const double *X, int64_t ldx, int d, int64_t n_rows, double *mx, const double *sm, const double *wm,
                                 double *mean, double *llks, int n_cu, hipStream_t s);
hipError_t launch_mix_loo_var(const double *X, int64_t ldx, int d, int64_t n_rows, const double *logpost, int c, int nm,
                              const double *m, const double *v, const double *ell, const double *L, const double *mean, double *var,
                              int first, hipStream_t s);

// held-out scoring (ppca_heldout.hip).  launch_holdout: train / held (n x d each) = the split of X by the
// counter-based generator (stream 8, keyed by row_offset + row and column); part[grid][2] = the workgroups' [kept, held] counts
// (reduce with launch_reduce_partials); grid = holdout_grid.  launch_heldout_score: the predictive log-density of the finite entries
// of H (a chunk's rows of `held`) under the rows' posteriors (states, covs: what the posterior pass wrote for the same rows of
// `train`); per_row (nullable) = the row's sum; part[grid][heldout_part_len(d, k)] = [w | w l | w e^2 | w e^2 / v (d each) | entries |
// rows with an entry | (scratch)] per workgroup (reduce with launch_reduce_partials; the first 4 d + 2 are the sums); grid =
// heldout_score_grid.
int holdout_grid(int64_t n, int d, int n_cu);
hipError_t launch_holdout(const double *X, int64_t ldx, int64_t n, int d, double lo, double hi, uint64_t seed, int64_t row_offset,
                          double *train, double *held, double *part, int grid, hipStream_t s);  // held iff lo <= u < hi
size_t heldout_score_lds_bytes(int d, int k);
int64_t heldout_part_len(int d, int k);
int heldout_score_grid(int64_t n_rows, int d, int k, int n_cu);
hipError_t launch_heldout_score(const double *H, int64_t ldh, const double *w, int d, int k, int64_t n_rows, const double *model,
                                const double *states, const double *covs, double *per_row, double *part, int grid, hipStream_t s);
// The mixture (chunk-local buffers): launch_heldout_fold folds component comp's (m, v, l) of every held entry into fold (5 arrays of
// n_rows x d: running maximum and scaled sum of lp_c + l_c, sum a_c (m_c - x), sum a_c v_c, sum a_c (m_c - x)^2; comp 0 initialises);
// launch_heldout_finish sums l = mx + ln sm, e^2 = A^2, e^2 / (V + max(Q - A^2, 0)) as launch_heldout_score does (part:
// heldout_part_len(d, 0), grid = heldout_score_grid(n_rows, d, 0, n_cu)).
hipError_t launch_heldout_fold(const double *H, int64_t ldh, int d, int k, int64_t n_rows, const double *model, const double *states,
                               const double *covs, const double *logpost, int comp, int nm, double *fold, int grid, hipStream_t s);
hipError_t launch_heldout_finish(const double *H, int64_t ldh, const double *w, int d, int64_t n_rows, const double *fold,
                                 double *per_row, double *part, int grid, hipStream_t s);
// The family arms of launch_heldout_score (heldout_family_covers: 1 <= k <= 16, 1 <= d <= 1024, else
// hipErrorInvalidValue).  _prec: Q = the chunk's rows of the held precisions; an entry is scored iff x is finite and q is finite and
// > 0, with v = sigma^2 / q + c_j^T Sigma c_j; states / covs: the known-precision posterior of the train rows (launch_hetero_sweep).
// _t: T = the chunk's rows of `train` (the kernel takes m and delta of the row from them), states / covs the Gaussian posterior,
// tbl[0 .. d] the device copy of ppca_t_pred_table_host.  part[grid][heldout_family_part_len(d, prec)] = [the 4 d sums | entries |
// rows with an entry | _prec: held precisions that are negative or +inf at a finite x]; grid = heldout_family_grid.
bool heldout_family_covers(int d, int k);
int64_t heldout_family_part_len(int d, bool prec);
int heldout_family_grid(int64_t n_rows, int n_cu);
hipError_t launch_heldout_score_prec(const double *H, int64_t ldh, const double *Q, int64_t ldq, const double *w, int d, int k,
                                     int64_t n_rows, const double *model, const double *states, const double *covs, double *per_row,
                                     double *part, int grid, hipStream_t s);
hipError_t launch_heldout_score_t(const double *H, int64_t ldh, const double *T, int64_t ldt, const double *w, int d, int k,
                                  int64_t n_rows, const double *model, const double *states, const double *covs, const double *tbl,
                                  double dof, double *per_row, double *part, int grid, hipStream_t s);
// per-column streaming passes of factor analysis (ppca_scale.hip).  launch_scale_columns: out (nullable, n x d)
// = x a_j on observed entries, NaN elsewhere; part[grid][3 d] the workgroups' column sums tot / sum / sq of w m, w m (x a - b),
// w m (x a - b)^2 (reduce with launch_reduce_partials); rowsum (nullable, n) = sum_j m_ij l_j; abl_dev = [a | b | l], 3 d doubles;
// grid = scale_grid(n, d, n_cu).  launch_fill_masked: out = x where observed (bit-exact), fill a_j elsewhere.
int scale_grid(int64_t n, int d, int n_cu);
hipError_t launch_scale_columns(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *abl_dev, double *out,
                                double *part, int grid, double *rowsum, hipStream_t s);
hipError_t launch_fill_masked(const double *X, int64_t ldx, const double *F, int64_t ldf, int64_t n, int d, const double *a_dev,
                              double *out, int n_cu, hipStream_t s);
// The same three column sums for nc row-weight vectors e_dev[nc][n] (instead of the dataset's weights) and nc offset vectors
// b_dev[nc][d] in one sweep (a_dev nullable = 1): part[grid][nc][3][d], grid = moments_multi_grid(n, nc, n_cu);
// reduce with launch_reduce_partials over nc * 3 * d.
int moments_multi_grid(int64_t n, int nc, int n_cu);
hipError_t launch_column_moments_multi(const double *X, int64_t ldx, int64_t n, int d, const double *e_dev, int nc, const double *a_dev,
                                       const double *b_dev, double *part, int grid, hipStream_t s);

// masked k-means (ppca_kmeans.hip).  launch_kmeans_assign: one sweep with the nc <= KMEANS_KB_MAX complete
// centres mu_dev[nc][d] (labels k0 .. k0 + nc) and the column scale a_dev (nullable = 1): labels / dist (nullable, n) = the nearest
// centre over the observed entries and its distance, the lowest index on a tie; carry: the minimum over the centre blocks before is in
// labels / dist.  accumulate (d <= 512, every centre in the launch): the workgroups' sums part[grid][plen] = [nc][2][d] tot / sum by
// label, from the same read of X.  inertia: the workgroups' sum_i w_i dist_i at part[.][plen - 1].  launch_kmeans_update: tot / sum of
// the centres k0 .. k0 + nc from the labels of an earlier sweep.  Reduce with launch_reduce_partials over plen; grid = kmeans_grid.
// launch_wd_block_sums: out[b] = sum of w_i dist_i (both nullable = 1) over the rows of block b (wd_block_rows() rows, wd_blocks(n)).
constexpr int KMEANS_KB_MAX = 8;
int kmeans_grid(int64_t n, int nc, int n_cu);
hipError_t launch_kmeans_assign(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *mu_dev, const double *a_dev,
                                int nc, int k0, int carry, int32_t *labels, double *dist, bool accumulate, double *part, int64_t plen,
                                int inertia, int grid, hipStream_t s);
hipError_t launch_kmeans_update(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *mu_dev, int nc, int k0,
                                const int32_t *labels, double *part, int64_t plen, int grid, hipStream_t s);
int64_t wd_blocks(int64_t n);
int64_t wd_block_rows();
hipError_t launch_wd_block_sums(const double *w, const double *dist, int64_t n, double *out, hipStream_t s);

// the Student-t sweep (ppca_robust.hip) over the n rows of a chunk whose posterior means (states, n x k) and
// Gaussian log-densities (llks, n) a posterior pass wrote: u, maha, ell (nullable, n) = the rows' weights, Mahalanobis distances and
// t log-densities; Y (nullable, n x d) = sqrt(u) (x - mean), NaN on masked entries; part[grid][plen], plen = robust_plen(d, k, sums
// || Y): the workgroups' column sums V (d x k) | A | T | sq (only with sums || Y) and the four scalars sum w | sum w ell |
// sum w (g[m] + ln u - u) | non-empty rows (reduce with launch_reduce_partials).  tabs = [lg (d + 1) | g (d + 1)] on the device
// (ppca_t_tables_host).  grid = robust_grid(n, d, k, n_cu).  Covers 1 <= k <= ROBUST_MAX_K, 1 <= d <= ROBUST_MAX_D.
constexpr int ROBUST_MAX_K = 16;    // k + 3 sums per column and the thread's rows of C live in registers
constexpr int ROBUST_MAX_D = 1024;  // four columns per thread of a 256-thread row
bool robust_covers(int d, int k);
int64_t robust_plen(int d, int k, bool sums);
int robust_grid(int64_t n, int d, int k, int n_cu);
hipError_t launch_robust_sweep(const double *X, int64_t ldx, const double *w, int64_t n, int d, int k, const double *model,
                               const double *llks, const double *states, const double *tabs, double nu, double *Y, bool sums, double *u,
                               double *maha, double *ell, double *part, int grid, hipStream_t s);

// heteroscedastic PPCA (ppca_hetero.hip): a precision p_ij per entry (P: a second n x d array; an entry is
// observed iff x is finite and p is finite and > 0).  launch_hetero_table: tab (d x hetero_ntp(k)) = [vech(c c^T) | C] of the model,
// zero-padded to 16-column blocks.  launch_hetero_sweep over the n rows of a chunk: llks (n), states (n x k), covs (n x k x k), rec
// (n x hetero_nrp(k): the records [w z | w | w (Sigma + z z^T) packed | 0 ..] the statistics kernel reads), all nullable;
// scal_part[grid][4] = the workgroups' sum w | sum w ell | non-empty rows | precisions that are negative or +inf (reduce with
// launch_reduce_partials); grid = hetero_sweep_grid(n, n_cu).  launch_hetero_stats: part[p.nsplit][hetero_stats_len(d, k)], the row
// runs' partials of cross (d x k) | S (d x k') | V (d x k) | A | T | sq | cnt (reduce with launch_reduce_partials over p.nsplit).
// launch_hetero_recon: out (n x d) = mean + C z (mode 0) or the observed value where observed (mode 1).
constexpr int HETERO_MAX_K = 16;
constexpr int HETERO_MAX_D = 1024;
struct HeteroPlan {
    int tiles, nsplit, nsplit_max;  // nsplit_max: what nsplit cannot exceed for any n on this device (the size of `part`)
    int64_t rows_per;
};
bool hetero_covers(int d, int k);
int hetero_ntp(int k);
int hetero_nrp(int k);
int64_t hetero_stats_len(int d, int k);
int hetero_sweep_grid(int64_t n, int n_cu);
HeteroPlan hetero_stats_plan(int64_t n, int d, int n_cu);
hipError_t launch_hetero_table(const double *model, int d, int k, double *tab, hipStream_t s);
hipError_t launch_hetero_sweep(const double *X, int64_t ldx, const double *P, int64_t ldp, const double *w, int64_t n, int d, int k,
                               const double *model, const double *tab, double *llks, double *states, double *covs, double *rec,
                               double *scal_part, int grid, hipStream_t s);
hipError_t launch_hetero_stats(const double *X, int64_t ldx, const double *P, int64_t ldp, int64_t n, int d, int k, const double *model,
                               const double *rec, const HeteroPlan &p, double *part, hipStream_t s);
hipError_t launch_hetero_recon(const double *X, int64_t ldx, const double *P, int64_t ldp, int64_t n, int d, int k, const double *model,
                               const double *states, int mode, double *out, int n_cu, hipStream_t s);

// pairwise second moments (ppca_moments.hip): sums = X~^T diag(w) X~, counts = M^T diag(w) M and (cross
// nullable) cross = X~^T diag(w) M, d x d row-major each, x~ = x - center on observed entries.  A job = (pair of 64-column tiles,
// I <= J) x (run of rows); its partials go to part (p.scratch_bytes) and a second kernel adds the runs in order and mirrors the
// upper triangle of sums / counts.  moments_plan takes the number of runs from n_cu; n = 0 launches nothing (nsplit = 0).
struct MomentsPlan {
    int tiles, npairs, nsplit, nq;
    int64_t rows_per;
    size_t scratch_bytes;
};
MomentsPlan moments_plan(int64_t n, int d, int n_cu, bool cross);
hipError_t launch_pairwise_moments(const double *X, int64_t ldx, const double *w, int64_t n, int d, const double *center_dev,
                                   const MomentsPlan &p, double *part, double *sums, double *counts, double *cross, hipStream_t s);

// mixture helpers
// llk: [n_models][n]; logw: [n_models]; w nullable.  Writes u: [n_models][n] =
// ln w_i + log posterior_ic (-inf when w_i <= 0) and lse[n] (mixture llk per sample).
hipError_t launch_mix_accumulate(double *out, const double *a, const double *dev, const double *mean,
                                 const double *logpost, int c, int nm, int64_t n, int d, int first, hipStream_t s);
hipError_t launch_mix_posteriors(const double *llk, const double *logw_dev, const double *w, int64_t n, int nm,
                                 double *u, double *lse, double *logpost, hipStream_t s);
hipError_t launch_reduce_max(const double *v, int64_t n, double *out_scalar, double *work, hipStream_t s);
// out[i] = exp(v[i] - *max_dev)
hipError_t launch_exp_shift(const double *v, const double *max_dev, int64_t n, double *out, hipStream_t s);
hipError_t launch_reduce_sum(const double *v, const double *w, int64_t n, double *out_scalar, double *work,
                             hipStream_t s, const int *n_dev = nullptr);  // n_dev: the element count lives on the device (n = upper bound)
hipError_t launch_mix_shift(double *mx, int nm, hipStream_t s);  // non-finite maxima -> 0 (mix.rs:312-323), in place
// out[0 .. nm) = log_softmax(ln sums + shift) (mix.rs:324-325, :335), out[nm] = *llk (nullable)
hipError_t launch_mix_logweights(const double *sums, const double *shift, const double *llk, int nm, double *out, hipStream_t s);
// rows[0 .. m) = ascending indices i with exp(v[i] - *shift_dev) > 0, wout[0 .. m) those weights, counts[select_blocks(n)] = m
// (counts: select_blocks(n) + 1 ints of scratch).
hipError_t launch_select_positive(const double *v, const double *shift_dev, int64_t n, int *counts, int *rows, double *wout,
                                  hipStream_t s);
int select_blocks(int64_t n);
// The same for nm components at once (one launch per stage instead of one per component and stage):
//   launch_mix_posteriors2   u, lse as launch_mix_posteriors + per-block partials bpart[nm + 1][select_blocks(n)]: the block maxima of
//                            u_c (NaNs skipped) and the block sums of w_i lse_i; launch_mix_stage2 reduces them in a fixed order into
//                            maxima[nm] and *llk_out.
//   launch_select_multi      counts[nm][nb + 1] (-> exclusive offsets, total at [nb]), rows[nm][n], wout[nm][n] as
//                            launch_select_positive per component, and the sums of the kept weights into sums_out[nm], the row
//                            counts into used_out[nm] (fixed order: per-block sums in wpart[nm][nb], then one workgroup per component).
hipError_t launch_mix_posteriors2(const double *llk, const double *logw_dev, const double *w, int64_t n, int nm, double *u, double *lse,
                                  double *bpart, hipStream_t s);
hipError_t launch_mix_stage2(const double *bpart, int64_t n, int nm, double *maxima, double *llk_out, hipStream_t s);
hipError_t launch_select_multi(const double *u, const double *shift_dev, int64_t n, int nm, int *counts, int *rows, double *wout, double *wpart,
                               double *sums_out, int *used_out, hipStream_t s);

}  // namespace ppca
