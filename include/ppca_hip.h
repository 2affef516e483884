/*
 * ppca_hip.h -- C-ABI of the MI355X-native PPCA EM engine (libppca_hip.so).
 *
 * This is the drop-in boundary for ONE path of viodotcom/ppca_rs: the EM hot path
 * (per-sample masked posterior inference + M-step sufficient statistics) and the
 * passes that share its per-sample math (llk / llks / infer / smooth /
 * extrapolate).  The reference has no FFI seam of its own: its only boundary is
 * the PyO3 class surface (src/python_bindings.rs:15-26).  Each entry point below
 * names the reference item it replaces (paths relative to the reference root);
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; opaque handles own device memory
 *   - every function returns 0 (PPCA_OK) or a negative ppca_status; the message of
 *     the last failure on the calling thread is ppca_last_error()
 *   - "host" pointers are caller-owned host memory; "dev" pointers are device
 *     memory on the context's GPU (e.g. a torch tensor's data_ptr())
 *   - matrices are row-major float64; transform C is (d x k), mean is (d)
 *   - a dataset entry is OBSERVED iff it is finite (dataset.rs:19-22); masked
 *     entries keep their non-finite value in device memory and are removed by
 *     selection, never by multiplication (utils.rs:118-127)
 *   - all work is enqueued on the context's stream; entry points that return
 *     host values synchronise that stream, the *_async/_dev ones do not
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     fails with PPCA_ERR_HIP
 */
#ifndef PPCA_HIP_H
#define PPCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPCA_ABI_VERSION 6

typedef enum ppca_status {
    PPCA_OK = 0,
    PPCA_ERR_INVALID = -1,     /* bad argument / shape mismatch (reference: panics, output_covariance.rs:124) */
    PPCA_ERR_HIP = -2,         /* HIP runtime failure or no device */
    PPCA_ERR_UNSUPPORTED = -3, /* (d, k) outside what the kernels cover */
    PPCA_ERR_EMPTY = -4,       /* empty dataset (reference: assert, ppca_model.rs:52; expect :358) */
    PPCA_ERR_NUMERIC = -5      /* e.g. singular mean-prior covariance (prior.rs:40) */
} ppca_status;

typedef struct ppca_ctx ppca_ctx;         /* one GPU + one stream */
typedef struct ppca_dataset ppca_dataset; /* device-resident Dataset (dataset.rs:93-100) */
typedef struct ppca_model ppca_model;     /* device-resident PPCAModel (ppca_model.rs:18-22,40) */

/* Prior (prior.rs:8-15).  Host pointers; mean is (d), mean_covariance is (d x d). */
typedef struct ppca_prior {
    int32_t has_mean_prior;            /* with_mean_prior            prior.rs:32-45 */
    const double *mean;
    const double *mean_covariance;
    int32_t has_isotropic_noise_prior; /* with_isotropic_noise_prior prior.rs:49-56 */
    double isotropic_noise_alpha;
    double isotropic_noise_beta;
    double transformation_precision;   /* with_transformation_precision prior.rs:60-65 */
} ppca_prior;

/* Synthetic data = the model's own generative process (sample_one,
 * ppca_model.rs:164-181): y = C n1 + mean + sigma n2, entry dropped with
 * probability mask_prob (mask_kind 0) or one cyclic run of mask_run dims per
 * sample (mask_kind 1).  Counter-based RNG keyed by (seed, GLOBAL row, column):
 * a shard [row_offset, row_offset + n_rows) of the same seed holds the same rows
 * whatever the number of shards. */
typedef struct ppca_synth_spec {
    int64_t row_offset;
    int64_t n_rows;
    int32_t d;
    int32_t k;
    double sigma;
    double mask_prob;
    int32_t mask_kind;
    int32_t mask_run;
    uint64_t seed;
    const double *transform; /* host (d x k) ground-truth C */
    const double *mean;      /* host (d) */
} ppca_synth_spec;

/* ------------------------------------------------------------------ misc */
const char *ppca_last_error(void);
int32_t ppca_abi_version(void);
/* 1 when (d, k) runs on the fused single-pass kernel, 0 when it runs on the
 * generic split pipeline, negative if unsupported. */
int32_t ppca_path_kind(int32_t d, int32_t k);

/* --------------------------------------------------------------- context */
/* device_id < 0: use the current HIP device.  stream: a hipStream_t to enqueue
 * on (NULL = the library creates its own).  Replaces rayon's process-global pool
 * (rayon parallel iterators, ppca_model.rs:221-227 et al.). */
int ppca_ctx_create(int32_t device_id, void *stream, ppca_ctx **out);
int ppca_ctx_destroy(ppca_ctx *ctx);
int ppca_ctx_set_stream(ppca_ctx *ctx, void *stream);
int ppca_ctx_synchronize(ppca_ctx *ctx);
/* Device blocks released by a context's buffers (output datasets, scratch) are kept
 * for its next allocation of about the same size instead of going through
 * hipFree / hipMalloc (0.2-0.4 s a pair at 8 GB, 30x the kernel that fills them);
 * at most PPCA_POOL_GB GiB (default min(32, an eighth of the device); 0 disables).
 * The cache is invisible to other allocators of the process (torch's): trim before large allocations made elsewhere.
 * ppca_ctx_trim returns the kept blocks to the device now; an allocation hipMalloc
 * refuses for lack of memory does the same for every context before retrying. */
int ppca_ctx_trim(ppca_ctx *ctx, int64_t *released_bytes);
/* When enabled, the library brackets every launch of the dominant EM kernel with
 * HIP events on the context stream; ppca_ctx_kernel_time returns the summed
 * duration and launch count since the last reset (synchronises). */
int ppca_ctx_enable_timing(ppca_ctx *ctx, int32_t enabled);
int ppca_ctx_kernel_time(ppca_ctx *ctx, double *total_ms, int64_t *launches, int32_t reset);

/* --------------------------------------------------------------- dataset */
/* Dataset(ndarray, weights=None)  src/python_bindings.rs:34-64.
 * x: (n x d) float64 with element strides (row_stride, col_stride) in ELEMENTS
 * (numpy views of any layout, :45); weights: n or NULL (= 1.0, dataset.rs:153-158). */
int ppca_dataset_from_host(ppca_ctx *ctx, const double *x, int64_t n, int32_t d, int64_t row_stride,
                           int64_t col_stride, const double *weights, ppca_dataset **out);
/* Borrow device memory (row-major n x d, weights n or NULL); not freed by the library. */
int ppca_dataset_from_device(ppca_ctx *ctx, const double *x_dev, int64_t n, int32_t d, const double *weights_dev,
                             ppca_dataset **out);
/* PPCAModel::sample (ppca_model.rs:186-191) with a seed, generated on device. */
int ppca_dataset_generate(ppca_ctx *ctx, const ppca_synth_spec *spec, ppca_dataset **out);
/* Dataset::with_weights dataset.rs:171-176: shares the rows, new weights (host or device). */
int ppca_dataset_with_weights(ppca_dataset *ds, const double *weights_host, const double *weights_dev,
                              ppca_dataset **out);
/* DatasetChunks src/python_bindings.rs:151-165: rows [start, start+len), shares storage. */
int ppca_dataset_slice(ppca_dataset *ds, int64_t start, int64_t len, ppca_dataset **out);
/* Dataset.concat src/python_bindings.rs:121-133 */
int ppca_dataset_concat(ppca_ctx *ctx, ppca_dataset *const *parts, int32_t n_parts, ppca_dataset **out);
int ppca_dataset_free(ppca_dataset *ds);
int64_t ppca_dataset_len(const ppca_dataset *ds);        /* __len__ :94-96 */
int32_t ppca_dataset_output_size(const ppca_dataset *ds); /* output_size :98-100 */
const double *ppca_dataset_device_x(const ppca_dataset *ds);
const double *ppca_dataset_device_weights(const ppca_dataset *ds);
/* Dataset.numpy :81-92 / masked_vector dataset.rs:64-72: masked entries come back NaN. */
int ppca_dataset_to_host(ppca_dataset *ds, double *out);
int ppca_dataset_weights_to_host(ppca_dataset *ds, double *out); /* weights :106-108 */
/* Dataset::empty_dimensions dataset.rs:194-222: flags[j] = 1 iff dim j is masked in every sample. */
int ppca_dataset_empty_dimensions(ppca_dataset *ds, int32_t *flags);

/* ----------------------------------------------------------------- model */
/* PPCAModel::new ppca_model.rs:43-48 (isotropic_noise = sigma, transform d x k, mean d). */
int ppca_model_create(ppca_ctx *ctx, int32_t d, int32_t k, double sigma, const double *transform,
                      const double *mean, ppca_model **out);
/* An uninitialised model buffer of the given shape (target of ppca_em_finalize). */
int ppca_model_alloc(ppca_ctx *ctx, int32_t d, int32_t k, ppca_model **out);
int ppca_model_download(ppca_model *m, double *sigma, double *transform, double *mean);
int ppca_model_free(ppca_model *m);
int32_t ppca_model_output_size(const ppca_model *m);
int32_t ppca_model_state_size(const ppca_model *m);

/* ------------------------------------------------- EM step (the hot path) */
/* Packed sufficient statistics of one shard (all linear in the sample weights,
 * hence additive across GPUs -- the ONE collective of the path is a sum of this
 * buffer).  k' = k(k+1)/2, symmetric entries lower-packed (e = a(a+1)/2 + b, b <= a):
 *   cross [d*k]   sum_i w_i x~_ij z_i              ppca_model.rs:281-293
 *   S     [d*k']  sum_i w_i m_ij (z_i z_i^T + Sigma_i)   :297-306
 *   U     [d*k]   sum_i w_i m_ij z_i               (for total_deviation, :338-347)
 *   sumx  [d]     sum_i w_i x~_ij
 *   totals[d]     sum_i w_i m_ij                   :348
 *   scalars[8]    square_error (:345), deviations_square_sum (:346),
 *                 llk of the INPUT model (:142-149), sum_i w_i, #non-empty samples, 0, 0, 0
 * with x~ = x - mean on observed dims (0 elsewhere), z_i/Sigma_i the posterior of
 * the INPUT model (infer_one :195-208). */
int64_t ppca_stats_len(int32_t d, int32_t k);

/* E-step + all M-step reductions over the dataset's rows in ONE streaming pass
 * (replaces infer :221-227 + the four sweeps of iterate_with_prior :278-358).
 * stats_dev: device buffer of ppca_stats_len doubles, overwritten.  Asynchronous. */
int ppca_em_accumulate(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double *stats_dev);
/* M-step finalisation on device from (all-reduced) statistics: d row solves
 * (:309-322, keep the old row when the system is singular), sigma^2 (:360-371),
 * mean (:373-377); prior hooks :307-308, :367-368, :379-384.  Asynchronous
 * unless a mean prior is given.  out may not alias model_in. */
int ppca_em_finalize(ppca_ctx *ctx, const ppca_model *model_in, const double *stats_dev, const ppca_prior *prior,
                     ppca_model *out);
/* Same arithmetic on host buffers (no GPU needed): used after a CPU-side
 * reduction and by the mean-prior branch. */
int ppca_em_finalize_host(int32_t d, int32_t k, double sigma, const double *transform, const double *mean,
                          const double *stats, const ppca_prior *prior, double *sigma_out, double *transform_out,
                          double *mean_out);
/* PPCAModel::iterate / iterate_with_prior (ppca_model.rs:267-269, :277-393;
 * src/python_bindings.rs:496-507) on a single GPU = accumulate + finalize.
 * llk_in (nullable): log-likelihood of model_in, a by-product of the pass
 * (saves the trainer's extra llk sweep, python/ppca_rs/__init__.py:51).
 * Reading llk_in synchronises; with llk_in == NULL the call is asynchronous. */
int ppca_em_step(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model_in, const ppca_prior *prior,
                 ppca_model *out, double *llk_in);
/* The log-likelihood by-product of the most recent ppca_em_step / ppca_em_step_sharded / ppca_em_step_group on
 * this context (the llk of THAT step's input model, over all shards), for callers that ran the step
 * asynchronously.  Synchronises. */
int ppca_em_last_llk(ppca_ctx *ctx, double *llk);
/* Debug/parity: the packed statistics copied to host. */
int ppca_stats_raw(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double *stats_host);

/* ------------------------------------------------ passes sharing the math */
/* PPCAModel::llk :142-149 (weighted total) and llks :152-159 (per sample,
 * unweighted; nullable; host or device destination). */
int ppca_llk(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double *total_host, double *per_sample_host);
int ppca_llks_dev(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double *per_sample_dev);
/* PPCAModel::infer :221-227 -> InferredMasked.states (n x k) and covariances
 * (n x k x k, nullable)  src/python_bindings.rs:211-234. */
int ppca_infer(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double *states_host, double *covs_host);
/* PPCAModel::smooth :237-244 (mode 0) / extrapolate :254-261 (mode 1): a new,
 * fully-unmasked dataset carrying the input weights (:259). */
int ppca_reconstruct(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, int32_t mode, ppca_dataset **out);
/* InferredMasked::smoothed_covariance_diagonal :485-508 (mode 0) and
 * extrapolated_covariance_diagonal :542-577 (mode 1; observed dims -> 0). */
int ppca_covariance_diagonal(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, int32_t mode,
                             ppca_dataset **out);

/* Posterior sampling / multiple imputation (PosteriorSampler, ppca_model.rs:597-626, without the host round trip): for every
 * row i, with z_i, Sigma_i the posterior of ppca_infer and U_i the upper-triangular factor of Sigma_i = U_i U_i^T,
 *   mode 0 (sample): x_i = C (z_i + U_i eps_i) + mean + sigma eta_i on every dimension;
 *   mode 1 (impute): observed entries passed through bit-exactly, masked ones the mode-0 value (one multiple-imputation draw).
 * eps_i (k) and eta_i (d) are standard normals of a counter-based generator keyed by (seed, stream, row_offset + i, index)
 * (DESIGN.md 4.9): the draws do not depend on the grid, chunking or path, and a shard with the right row_offset reproduces
 * the single-device rows.  A new fully observed dataset carrying the input weights. */
int ppca_posterior_sample(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, int32_t mode, uint64_t seed,
                          int64_t row_offset, ppca_dataset **out);

/* Entry-wise hold-out (Wold's cross-validation split) on the device, in one streaming pass (an extension with no reference
 * counterpart).  Entry (i, j) of global row g = row_offset + i draws u = (word >> 11) 2^-53 in [0, 1) from the
 * counter-based generator of ppca_posterior_sample, stream 8: word = row_word(row_key(seed, 8, g), j).  An observed
 * (finite) entry is HELD iff u < fraction: it becomes NaN in train and keeps its bits in held; a kept entry keeps its bits in train
 * and becomes NaN in held; a masked entry is NaN in both.  Both outputs are new datasets carrying the input weights.  fraction = 0
 * holds nothing, fraction = 1 every observed entry; a fraction outside [0, 1] or NaN is PPCA_ERR_INVALID.  counts_host (nullable, 2) =
 * [entries kept, entries held], unweighted.  Nothing depends on the grid; a shard with the right row_offset reproduces the
 * single-device rows. */
int ppca_dataset_holdout(ppca_ctx *ctx, ppca_dataset *ds, double fraction, uint64_t seed, int64_t row_offset, ppca_dataset **train_out,
                         ppca_dataset **held_out, double *counts_host);
/* The same split with the held entries those of lo <= u < hi (the same u): ppca_dataset_holdout(fraction) is the range (0, fraction),
 * bit for bit.  Ranges that share their edges -- (f / K, (f + 1) / K) for f = 0 .. K - 1, the last edge exactly 1 -- are K disjoint
 * folds that hold every observed entry exactly once.  Requires 0 <= lo <= hi <= 1; anything else, or NaN, is PPCA_ERR_INVALID. */
int ppca_dataset_holdout_range(ppca_ctx *ctx, ppca_dataset *ds, double lo, double hi, uint64_t seed, int64_t row_offset,
                               ppca_dataset **train_out, ppca_dataset **held_out, double *counts_host);
/* The predictive log-density of held-out entries.  With (z, Sigma) the posterior of row i given its entries in
 * `train` (ppca_infer), every finite entry x of `held` in that row is scored as a NEW reading of column j:
 *   m = mean_j + c_j^T z,  v = sigma^2 + c_j^T Sigma c_j,  e = x - m,  l = -1/2 (ln 2 pi + ln v + e^2 / v)
 * whatever `train` holds at j: the two datasets need equal shape (else PPCA_ERR_INVALID) but no particular relation.  A row without
 * entries in train gets the prior predictive (mean_j, sigma^2 + |c_j|^2), state size 0 gives (mean_j, sigma^2).  Weights are train's.
 *   per_row (nullable, n; host or device as ppca_llk's per-sample output): sum_j l, 0 for a row without held entries
 *   totals_host (6): sum_i w_i n_i, sum w l, sum w e^2, sum w e^2 / v (each the column sums added in index order), the unweighted
 *                    entry count, the rows with at least one held entry
 *   col_sums_host (nullable, 4 d): per column the weighted count, sum w l, sum w e^2, sum w e^2 / v
 * No N x d buffer is allocated or written.  per_row depends on its row alone (bit-identical across grids, chunks and slices); the
 * sums are bit-reproducible for a given grid (fixed-order partials, no float atomics). */
int ppca_heldout_score(ppca_ctx *ctx, ppca_dataset *train, ppca_dataset *held, const ppca_model *model, double *totals_host,
                       double *col_sums_host, double *per_row);

/* Leave-one-out predictive of every entry (an extension with no reference counterpart): for each entry j of row i,
 * the predictive of x_ij given the row's OTHER observed entries, the model held fixed.  With z, Sigma the row's posterior (ppca_infer),
 * r_j = x_j - mean_j - c_j^T z, q_j = c_j^T Sigma c_j and s_j = sigma^2 - q_j:
 *   observed j: mean x_j - sigma^2 r_j / s_j, variance sigma^4 / s_j, log-density l_j = -1/2 (log 2 pi + log(sigma^4 / s_j) + r_j^2 / s_j)
 *   masked j:   mean mean_j + c_j^T z (ppca_reconstruct mode 1), variance sigma^2 + q_j (ppca_covariance_diagonal mode 1)
 * An observed entry whose s_j rounding took to sigma^4 / (sigma^2 + |c_j|^2) or below (the exact value is never below) gets the
 * prior predictive (mean_j, sigma^2 + |c_j|^2).  per_sample_host[i] = sum of l_j over the row's observed entries (0 for a row with
 * none), total_host = sum_i w_i per_sample_host[i].  mean_out / var_out: new fully observed datasets carrying the input weights.
 * Every output is nullable, at least one is given; with both dataset outputs null no N x d buffer is allocated or written. */
int ppca_loo_predictive(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, ppca_dataset **mean_out, ppca_dataset **var_out,
                        double *total_host, double *per_sample_host);

/* ------------------------------------- factor analysis: per-column noise */
/* An extension with no reference counterpart: x = C z + mean + eps with eps_j ~ N(0, psi_j^2), one noise level per column.  Dividing
 * column j by s_j = psi_j turns it into the isotropic model: with A = diag(1/s) C, mean~ = mean / s and Y = X diag(1/s) (masked
 * entries stay masked), PPCAModel(1, A, mean~) on Y has the posterior (z_i, Sigma_i) of the FA model on X, and
 * llks_FA(x_i) = llks_PPCA(y_i) - sum_{j observed in i} ln s_j.  An FA model is three host arrays: noise (d), transform (d x k), mean (d).
 *
 * ppca_dataset_scale_columns: one streaming pass over the dataset with per-column host vectors a, b, l (d each; b, l nullable = 0):
 *   out     (nullable) a new dataset carrying the input weights: x_ij a_j (one fp64 multiply) on observed entries, NaN on masked
 *           ones; with out == NULL no N x d buffer is allocated or written
 *   col_sums_host (nullable, 3 d): tot_j = sum_i w_i m_ij | sum_j = sum_i w_i m_ij (x_ij a_j - b_j) | sq_j = sum_i w_i m_ij (x_ij a_j - b_j)^2
 *   row_sums (nullable, n; host or device, as ppca_llk's per-sample output): sum_j m_ij l_j
 * Column sums go through per-workgroup partials added in a fixed order (no float atomics): bit-reproducible for a given grid; out
 * and row_sums do not depend on the grid at all.  At least one output is given.  Synchronises. */
int ppca_dataset_scale_columns(ppca_ctx *ctx, ppca_dataset *ds, const double *a_host, const double *b_host, const double *l_host,
                               ppca_dataset **out, double *col_sums_host, double *row_sums);
/* ppca_dataset_pairwise_moments: the second moments between every two columns over the entries that are there.  With
 * center_host (d, nullable = 0; every entry finite) and x~_ij = x_ij - center_j on observed entries, 0 on masked ones, three d x d
 * row-major host matrices:
 *   sums_host[j][l]   = sum_i w_i x~_ij x~_il   (only rows with both observed contribute)            symmetric
 *   counts_host[j][l] = sum_i w_i m_ij m_il                                                        symmetric
 *   cross_host[j][l]  = sum_i w_i x~_ij m_il    (centred column j over the rows where l is observed)   nullable, not symmetric
 * The centring happens before the product (a column with mean 1e6 and unit spread does not cancel) and the weights enter as in the
 * column sums of ppca_dataset_scale_columns: diag(counts) is that pass's tot and diag(sums) its sq for b = center.  sums / counts is the
 * covariance around a common centre; (sums - cross o cross^T / counts) / (counts - 1) is the pairwise-complete covariance.  Dense fp64
 * MFMA contractions over 64-column tile pairs I <= J x runs of rows, per-job partials added in a fixed order (no float atomics:
 * bit-reproducible for a given grid) and the upper triangle mirrored, so that sums and counts are symmetric bit for bit.  cross costs as
 * much as the other two together and is computed only when asked for.  An empty dataset gives zeros.  Scratch comes from the context's
 * block cache and does not grow with N.  Synchronises. */
int ppca_dataset_pairwise_moments(ppca_ctx *ctx, ppca_dataset *ds, const double *center_host, double *sums_host, double *counts_host,
                                  double *cross_host);
/* ------------------------------------- masked k-means */
/* ppca_dataset_kmeans_step: one Lloyd iteration.  centers_host (n_clusters x d, row-major, every entry finite), scale_host (d, nullable
 * = 1, finite), n_clusters in 1 .. 16 (PPCA_ERR_UNSUPPORTED outside; a non-finite centre or scale: PPCA_ERR_INVALID, before any launch).
 *   dist_ic   = sum_j m_ij (a_j (x_ij - mu_cj))^2     over the row's observed entries: difference, then scale, then square
 *   labels[i] = the SMALLEST c that attains min_c dist_ic (an exact tie goes to the lowest index; a row with no observed entry: 0)
 *   dist[i]   = that minimum                            labels, dist: n each, nullable, host or device destinations
 *   sums_host [n_clusters][2][d], nullable:  tot_cj = sum_{i: labels[i] = c} w_i m_ij | sum_cj = sum_{i: labels[i] = c} w_i m_ij (x_ij - mu_cj)
 *             (unscaled and centred on the OLD centre: nothing cancels).  The new centre is mu_cj + sum_cj / tot_cj where tot_cj > 0
 *             and mu_cj elsewhere: the caller divides.
 *   inertia_host (nullable) = sum_i w_i dist[i].  The dataset's weights enter sums and inertia, not the assignment.
 *   reads_host (nullable): the sweeps over X the call made -- 1 with d <= 512 and n_clusters <= 8 (the sums are taken from the read
 *             that assigns) and whenever sums_host is NULL and n_clusters <= 8; otherwise an assignment sweep per block of 8 centres
 *             plus, with sums_host, an update sweep per block.
 * Per-workgroup partials added in a fixed order (no float atomics): sums and inertia are bit-reproducible for a given grid; labels and
 * dist do not depend on the grid at all.  An empty dataset gives zeros and writes no labels.  Scratch comes from the context's block
 * cache: the partials and, when they are needed, the two per-row arrays.  Synchronises once. */
int ppca_dataset_kmeans_step(ppca_ctx *ctx, ppca_dataset *ds, const double *centers_host, const double *scale_host, int32_t n_clusters,
                             int32_t *labels, double *dist, double *sums_host, double *inertia_host, int32_t *reads_host);
/* ppca_dataset_kmeans_seed: k-means++ from n_clusters caller-drawn numbers u_host in [0, 1).  Centre 0 is the smallest row r with
 * cumsum(w)_r > u_0 sum(w); centre c >= 1 the smallest r with cumsum(w D)_r > u_c sum(w D), D_i the row's distance (as above) to the
 * nearest centre chosen so far (that total 0: the rule of centre 0).  A centre made from row r is x_rj where observed and the weighted
 * mean of column j over its observed entries (0 for an empty column) elsewhere.  The pick has two levels -- block sums of w D choose a
 * block of rows, then only that block's slice comes to the host.  n_clusters - 1 reads of X plus the mean sweep.  centers_host
 * (n_clusters x d); rows_host (n_clusters, nullable): the chosen rows.  An empty dataset: PPCA_ERR_EMPTY. */
int ppca_dataset_kmeans_seed(ppca_ctx *ctx, ppca_dataset *ds, const double *scale_host, int32_t n_clusters, const double *u_host,
                             double *centers_host, int64_t *rows_host);
/* out_ij = x_ij, bit-exact, where ds is observed; fill_ij a_j elsewhere (fill: a dataset of the same shape; a_host: d).  A new
 * dataset carrying the weights of ds: the last step of the FA model's extrapolate.  Synchronises. */
int ppca_dataset_fill_masked(ppca_ctx *ctx, ppca_dataset *ds, ppca_dataset *fill, const double *a_host, ppca_dataset **out);
/* The FA M-step on host buffers (no GPU needed, like ppca_em_finalize_host).  stats: the packed statistics of the EM pass of
 * PPCAModel(1, A, mean~) on Y; sq_j = sum_i w_i m_ij (y_ij - mean~_j)^2 (ppca_dataset_scale_columns with a = 1 / s, b = mean / s);
 * min_noise (d, nullable = 0).  Per column j, tot = totals_j -- an ECM step, each block maximised given the blocks already
 * updated, so the log-likelihood cannot decrease:
 *   1. a_j = solution of S_j a = cross_j by the Cholesky row solve; a pivot <= 0 keeps the old row c_j / s_j; no prior term
 *   2. delta_j = (sumx_j - a_j . U_j) / tot with the NEW a_j (0 if tot = 0); mean~_j += delta_j
 *   3. psi~_j^2 = (sq_j - 2 a_j . cross_j + a_j^T S_j a_j - delta_j^2 tot) / tot with the new a_j, delta_j; psi~_j = 1 if tot = 0 or the
 *      value is non-finite or <= 0
 *   4. c_j = s_j a_j, mean_j = s_j mean~_j, psi_j = max(s_j psi~_j, min_noise_j)
 * Outputs may not alias inputs. */
int ppca_fa_finalize_host(int32_t d, int32_t k, const double *noise, const double *transform, const double *mean, const double *stats,
                          const double *sq, const double *min_noise, double *noise_out, double *transform_out, double *mean_out);
/* One FA EM iteration on a single GPU: whiten + sq (ppca_dataset_scale_columns), ppca_em_accumulate on the whitened dataset, the
 * statistics to the host, ppca_fa_finalize_host; the whitened dataset is released before returning (peak device memory: twice the
 * dataset).  llk_in (nullable): log-likelihood of the INPUT FA model, the pass's by-product minus sum_j totals_j ln s_j.  One
 * synchronisation per call. */
int ppca_fa_em_step(ppca_ctx *ctx, ppca_dataset *ds, int32_t d, int32_t k, const double *noise, const double *transform,
                    const double *mean, const double *min_noise, double *noise_out, double *transform_out, double *mean_out,
                    double *llk_in);

/* ------------------------------------- mixture of factor analysers with shared column noise */
/* An extension with no reference counterpart (Ghahramani & Hinton's mixture of factor analysers): x | c = C_c z + mean_c + eps with
 * eps_j ~ N(0, psi_j^2) and P(c) = pi_c: ONE noise vector psi (d) for all components, per component a transform (d x k), a mean (d) and
 * a log-weight; all components have the same k.  With s = psi, Y = X diag(1/s), A_c = diag(1/s) C_c and mean~_c = mean_c / s the
 * mixture of PPCAModel(1, A_c, mean~_c) on Y has the component posteriors of the FA mixture on X, and
 * llks_FAMix(x_i) = logsumexp_c(log pi_c + llks_PPCA_c(y_i)) - sum_{j observed in i} ln s_j.  A model is four host arrays: noise (d),
 * transforms (n_comp x d x k), means (n_comp x d), log_weights (n_comp).
 *
 * ppca_dataset_column_moments_multi: one streaming pass over the dataset for n_comp (1 .. 16) row-weight vectors at once.  e (n_comp x n,
 * component-major; exactly one of e_host / e_dev is given, as ppca_dataset_with_weights) is used INSTEAD of the dataset's weights; a
 * non-finite weight counts as 0; a_host (d, nullable = 1); b_host (n_comp x d, nullable = 0).  sums_host [n_comp][3][d]:
 *   tot_cj = sum_i e_ci m_ij | sum_cj = sum_i e_ci m_ij (x_ij a_j - b_cj) | sq_cj = sum_i e_ci m_ij (x_ij a_j - b_cj)^2
 * each element centred on its own component's b_cj before it is squared.  a and b must be finite: the mask enters as a factor 0 on the
 * weight, so a masked entry adds exactly nothing only while its b_cj is finite (a non-finite offset turns the column's sums into NaN
 * even where every entry is masked, where ppca_dataset_scale_columns would give 0).  Up to 8 components the dataset is read once; 9 .. 16 take
 * the components in two blocks of 8, each over the rows again.  Per-workgroup partials added in a fixed order (no float atomics):
 * bit-reproducible for a given grid.  An empty dataset gives zeros.  Synchronises. */
int ppca_dataset_column_moments_multi(ppca_ctx *ctx, ppca_dataset *ds, const double *e_host, const double *e_dev, int32_t n_comp,
                                      const double *a_host, const double *b_host, double *sums_host);
/* The M-step of the FA mixture on host buffers (no GPU needed).  stats: n_comp packed buffers of ppca_stats_len(d, k), component c's the
 * statistics of the EM pass of PPCAModel(1, A_c, mean~_c) on Y under the row weights w_i r_ic; sq (n_comp x d): sq_cj = sum_i w_i r_ic m_ij
 * (y_ij - mean~_cj)^2; scale (n_comp, nullable = 1): a factor >= 0 on component c's statistics and sq before the components are pooled
 * (the component passes weight their rows by exp(u_ic - shift_c) with a shift per component: scale_c = exp(shift_c - max shift));
 * min_noise (d, nullable = 0).  An ECM step in ppca_fa_finalize_host's block order -- the log-likelihood cannot decrease.  Per column j:
 *   1. per component a_cj = solution of S_cj a = cross_cj by the Cholesky row solve; a pivot <= 0 keeps the old row; no prior term
 *   2. delta_cj = (sumx_cj - a_cj . U_cj) / totals_cj with the NEW a_cj (0 if totals_cj = 0); mean~_cj += delta_cj
 *   3. psi~_j^2 = sum_c scale_c (sq_cj - 2 a_cj . cross_cj + a_cj^T S_cj a_cj - delta_cj^2 totals_cj) / sum_c scale_c totals_cj;
 *      psi~_j = 1 if the denominator is 0 or the value is non-finite or <= 0
 *   4. C_cj = s_j a_cj, mean_cj = s_j mean~_cj, psi_j = max(s_j psi~_j, min_noise_j)
 * Outputs may not alias inputs. */
int ppca_famix_finalize_host(int32_t d, int32_t k, int32_t n_comp, const double *noise, const double *transforms, const double *means,
                             const double *stats, const double *sq, const double *scale, const double *min_noise, double *noise_out,
                             double *transforms_out, double *means_out);
/* One iteration of the FA mixture on a single GPU (n_comp <= 16), composed from existing passes and the sweep above: whiten + the
 * weighted column totals (ppca_dataset_scale_columns); the responsibilities of the whitened components on Y; per component the shift,
 * the gathered weighted EM pass of ppca_mix_em_step's component-by-component form and its weights exp(u_ic - shift_c) into a K x n
 * buffer; ppca_dataset_column_moments_multi's sweep on Y with a = 1, b_c = mean~_c; statistics to the host;
 * ppca_famix_finalize_host; log_weights_out = log_softmax_c(ln sum_i w_i r_ic).  Rows with w_i <= 0 contribute nothing.  llk_in
 * (nullable): log-likelihood of the INPUT model, sum_i w_i lse_i - sum_j tot_j ln s_j.  The whitened copy is released to the block
 * cache before returning (peak device memory: twice the dataset + 3 n_comp n doubles).  Three synchronisations per call: two inside
 * ppca_dataset_scale_columns, one for the results. */
int ppca_famix_em_step(ppca_ctx *ctx, ppca_dataset *ds, int32_t d, int32_t k, int32_t n_comp, const double *noise, const double *transforms,
                       const double *means, const double *log_weights, const double *min_noise, double *noise_out,
                       double *transforms_out, double *means_out, double *log_weights_out, double *llk_in);

/* --------------------------------------------------- Student-t PPCA for masked data */
/* An extension with no reference counterpart (Archambeau, Delannay and Verleysen's robust PPCA; the ECM of Lange, Little and Taylor):
 * x | u = C z + mean + eps with z ~ N(0, I / u), eps ~ N(0, sigma^2 I / u) and u ~ Gamma(nu / 2, rate nu / 2), so the observed part of a
 * row is multivariate t with nu degrees of freedom.  A model is (sigma, C, mean) -- an ordinary ppca_model -- and nu.  For a row with m
 * observed entries, posterior mean z (what ppca_infer returns: it does not depend on nu), x~ = x_O - mean_O and r = x~ - C_O z:
 *   delta = (|r|^2 + sigma^2 |z|^2) / sigma^2                 the Mahalanobis distance x~^T (C_O C_O^T + sigma^2 I)^-1 x~
 *   u     = (nu + m) / (nu + delta)                           the row's weight E[u | x]: small = outlying, at most (nu + m) / nu
 *   ell   = lg[m] - 1/2 logdet - 1/2 (nu + m) log1p(delta / nu)   the t log-density, logdet = (m - k) ln sigma^2 + ln det M
 * A row without an observed entry has delta = 0, u = 1, ell = 0.  Covers 1 <= k <= 16 and 1 <= d <= 1024 (PPCA_ERR_UNSUPPORTED beyond,
 * before any launch).
 *
 * ppca_t_tables_host: host only.  lg_out[m] = ln Gamma((nu + m) / 2) - ln Gamma(nu / 2) - (m / 2) ln(nu pi) and
 * g_out[m] = psi((nu + m) / 2) - ln((nu + m) / 2) for m = 0 .. d (d + 1 doubles each); std::lgamma (Stirling's series term by term from
 * nu >= 2e4 on, where the difference of the two values cancels), digamma by upward recurrence and its asymptotic series. */
int ppca_t_tables_host(int32_t d, double dof, double *lg_out, double *g_out);
/* ppca_t_estep: the posterior pass of ppca_infer / ppca_llk into (k + 1) doubles per row of scratch (by row chunks of at most 1 GiB), then
 * ONE streaming sweep over the dataset.  Every output is nullable; at least one must be given.
 *   scaled_out     a new dataset y_ij = sqrt(u_i) (x_ij - mean_j) -- bit for bit fl(fl(sqrt(u_i)) fl(x_ij - mean_j)) -- NaN on masked
 *                  entries, carrying the weights of ds; without it no n x d buffer is allocated or written
 *   col_sums_host  (k + 3) d doubles, V (d x k) | A (d) | T (d) | sq (d): V_j = sum_i w u m_ij z_i, A_j = sum w u m x~_j, T_j = sum w u m,
 *                  sq_j = sum w u m x~_j^2
 *   u, maha, llks  n doubles each: u_i, delta_i, ell_i (host or device destinations, as ppca_llk's per-sample output)
 *   scalars_host   4 doubles: sum w | sum w ell | sum w (g[m] + ln u - u) | rows with an observed entry
 * Per-workgroup partials added in a fixed order (no float atomics): the sums are bit-reproducible for a given grid; the per-row outputs
 * and the scaled rows do not depend on the grid, the chunks or a slice's offset.  An empty dataset gives zeros.  Synchronises once. */
int ppca_t_estep(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, double dof, ppca_dataset **scaled_out, double *col_sums_host,
                 double *u, double *maha, double *llks, double *scalars_host);
/* The ECM M-step on host buffers (no GPU needed, like ppca_fa_finalize_host).  stats: the packed statistics of the EM pass of
 * PPCAModel(sigma, C, 0) on the scaled rows Y of ppca_t_estep -- cross_j = sum w u m x~_j z, S_j = sum w m (Sigma + u z z^T),
 * totals_j = sum w m; col_sums: ppca_t_estep's.  Each block is maximised given the blocks already updated, so the t log-likelihood
 * cannot decrease.  Per column j:
 *   1. c_j = solution of S_j a = cross_j by the Cholesky row solve; a pivot <= 0 keeps the old row; no prior term
 *   2. delta_j = (A_j - c_j . V_j) / T_j with the NEW c_j (0 if T_j = 0); mean_j += delta_j
 *   3. sigma^2 = sum_j (sq_j - 2 c_j . cross_j + c_j^T S_j c_j - delta_j^2 T_j) / sum_j totals_j; a non-finite or non-positive value
 *      keeps the old sigma
 * This is not the reference's EM step (which uses the old C in its mean and noise updates); as nu -> infinity, u -> 1 and it becomes
 * the ECM step of ppca_fa_finalize_host's block order with one pooled noise.  Outputs may not alias inputs.  k >= 1. */
int ppca_t_finalize_host(int32_t d, int32_t k, double sigma, const double *transform, const double *mean, const double *stats,
                         const double *col_sums, double *sigma_out, double *transform_out, double *mean_out);
/* One Student-t ECM iteration on a single GPU: the sweep of ppca_t_estep with the scaled rows, ppca_em_accumulate on them with the
 * model (sigma, C, 0), statistics to the host, ppca_t_finalize_host; the scaled rows are released before returning (peak device memory:
 * twice the dataset).  llk_in (nullable): the t log-likelihood of the INPUT model, sum_i w_i ell_i; q_out (nullable):
 * q = sum w (g[m] + ln u - u) / sum w, with which the degrees of freedom are updated as the root of ln(nu / 2) - psi(nu / 2) + 1 + q = 0.
 * One synchronisation of its own per call (uploads and downloads are queued behind the kernels). */
int ppca_t_em_step(ppca_ctx *ctx, ppca_dataset *ds, int32_t d, int32_t k, double sigma, const double *transform, const double *mean,
                   double dof, double *sigma_out, double *transform_out, double *mean_out, double *llk_in, double *q_out);
/* ppca_heldout_score under the t model.  The observed part of a row and one further entry are jointly t, so given the
 * row's m train entries a held entry is univariate t with nu_m = nu + m degrees of freedom.  With (z, Sigma) the Gaussian posterior
 * given `train` (ppca_infer) and delta the row's distance given `train` (above; m = 0: delta = 0, z = 0, Sigma = I, the t prior
 * predictive):
 *   loc = mean_j + c_j . z,  s = (sigma^2 + c_j^T Sigma c_j) (nu + delta) / nu_m,  e = x - loc
 *   l   = tbl[m] - 1/2 ln s - 1/2 (nu_m + 1) log1p(e^2 / (nu_m s))
 *   tbl[m] = ln Gamma((nu_m + 1) / 2) - ln Gamma(nu_m / 2) - 1/2 ln(nu_m pi)
 * The fourth sum (e^2 / v) takes the variance v = s nu_m / (nu_m - 2); when nu_m <= 2 there is none and the entry adds 0 to it (it
 * still counts everywhere else).  Outputs, weights and the reproducibility contract are ppca_heldout_score's; no N x d buffer is
 * allocated.  Covers 1 <= k <= 16 and 1 <= d <= 1024.
 * ppca_t_pred_table_host: host only, tbl_out[m] for m = 0 .. d (d + 1 doubles); as ppca_t_tables_host, the difference of the two
 * ln Gamma is taken term by term of Stirling's series where the values themselves would cancel. */
int ppca_t_pred_table_host(int32_t d, double dof, double *tbl_out);
int ppca_t_heldout_score(ppca_ctx *ctx, ppca_dataset *train, ppca_dataset *held, const ppca_model *model, double dof,
                         double *totals_host, double *col_sums_host, double *per_row);

/* --------------------------------------------------- PPCA with a known precision per entry */
/* An extension with no reference counterpart (weighted / heteroscedastic PCA: Bailey's EMPCA, Delchambre's weighted PCA):
 *   x_ij = mean_j + c_j . z_i + eps_ij,   z_i ~ N(0, I_k),   eps_ij ~ N(0, sigma^2 / p_ij)
 * with p_ij > 0 the KNOWN precision of entry (i, j) relative to sigma^2; p = 1 everywhere is the model of ppca_llk / ppca_infer.  A
 * model is an ordinary ppca_model; the precisions are `prec`, a ppca_dataset of the same n and d as ds (its own row weights are
 * ignored; another shape: PPCA_ERR_INVALID).  Entry (i, j) is observed iff x_ij is finite and p_ij is finite and > 0: p_ij NaN or 0
 * means not observed, whatever x_ij holds.  A precision < 0 or = +inf is an error: the sweep counts them next to its scalars and the
 * call returns PPCA_ERR_INVALID after its own synchronisation, with no output written.  For row i with observed set O (m entries),
 * x~ = x - mean and the dataset's row weight w_i:
 *   G_i = sum_O p_ij c_j c_j^T     b_i = sum_O p_ij x~_ij c_j     M_i = sigma^2 I + G_i
 *   z_i = M_i^-1 b_i               Sigma_i = sigma^2 M_i^-1
 *   ell_i = -1/2 [ (sum_O p_ij x~_ij^2 - b_i^T M_i^-1 b_i) / sigma^2 + ln det M_i + (m - k) ln sigma^2 + m ln 2 pi - sum_O ln p_ij ]
 * A row with m = 0 has ell_i = 0 and z_i = 0.  Statistics of one E-step, per column j (ppca_h_stats_len(d, k) = d (2 k + k (k + 1) / 2 + 4)
 * doubles, in this order):
 *   cross_j = sum_i w_i p_ij x~_ij z_i  (d x k)            S_j = sum_i w_i p_ij (Sigma_i + z_i z_i^T)  (d x k (k + 1) / 2, lower-packed)
 *   V_j = sum_i w_i p_ij z_i  (d x k)                      A_j = sum_i w_i p_ij x~_ij  (d)             T_j = sum_i w_i p_ij  (d)
 *   sq_j = sum_i w_i p_ij x~_ij^2  (d)                     cnt_j = sum_i w_i m_ij  (d; m_ij = 1 where observed)
 * Covers 1 <= k <= 16 and 1 <= d <= 1024 (PPCA_ERR_UNSUPPORTED beyond, before any launch).  Everything is fp64 on v_mfma_f64_16x16x4:
 * a sweep over X and P forms [G | b] of 16 rows per wave against the table [vech(c c^T) | C] and solves one row per lane; the
 * statistics are a second read of X and P against the rows' records [w z | w | w (Sigma + z z^T)], which pass through at most 1 GiB of
 * scratch (row chunks; PPCA_H_CHUNK=rows in the environment forces a chunk length).  Per-workgroup partials added in a fixed order (no
 * float atomics); ell_i, z_i and Sigma_i depend on their row alone, not on the grid, the chunks or a slice's offset. */
int64_t ppca_h_stats_len(int32_t d, int32_t k);
/* The E-step.  Every output is nullable; at least one must be given.  llks (n), states (n x k), covs (n x k x k): host or device
 * destinations, as ppca_llk's per-sample output.  stats_host: the statistics above.  scalars_host: 4 doubles, sum w | sum w ell |
 * rows with an observed entry | the count of bad precisions (0 whenever the call succeeds).  An empty dataset gives zeros. */
int ppca_h_estep(ppca_ctx *ctx, ppca_dataset *ds, ppca_dataset *prec, const ppca_model *model, double *llks, double *states, double *covs,
                 double *stats_host, double *scalars_host);
/* mode 0 (smooth): out_ij = mean_j + c_j . z_i everywhere; mode 1 (extrapolate): x_ij, bit-exact, where entry (i, j) is observed by
 * the rule above, mean_j + c_j . z_i elsewhere.  A new dataset carrying the weights of ds. */
int ppca_h_reconstruct(ppca_ctx *ctx, ppca_dataset *ds, ppca_dataset *prec, const ppca_model *model, int32_t mode, ppca_dataset **out);
/* The ECM M-step on host buffers (no GPU needed), in the block order of ppca_t_finalize_host, all from one E-step, so that the
 * log-likelihood cannot decrease.  stats: ppca_h_estep's.  Per column j:
 *   1. c_j = solution of S_j a = cross_j by the Cholesky row solve; a pivot <= 0 keeps the old row
 *   2. delta_j = (A_j - c_j . V_j) / T_j with the NEW c_j (0 if T_j = 0); mean_j += delta_j
 *   3. sigma^2 = sum_j (sq_j - 2 c_j . cross_j + c_j^T S_j c_j - delta_j^2 T_j) / sum_j cnt_j -- the weighted COUNT of observed entries,
 *      not the sum of their precisions; a non-finite or non-positive value keeps the old sigma
 * Not the reference's EM step (the caveat of ppca_fa_finalize_host and ppca_t_finalize_host).  Outputs may not alias inputs. */
int ppca_h_finalize_host(int32_t d, int32_t k, double sigma, const double *transform, const double *mean, const double *stats,
                         double *sigma_out, double *transform_out, double *mean_out);
/* One ECM iteration on a single GPU: model upload, sweep, statistics contraction, one synchronisation, ppca_h_finalize_host.  llk_in
 * (nullable): the log-likelihood of the INPUT model, sum_i w_i ell_i, a by-product of the sweep. */
int ppca_h_em_step(ppca_ctx *ctx, ppca_dataset *ds, ppca_dataset *prec, int32_t d, int32_t k, double sigma, const double *transform,
                   const double *mean, double *sigma_out, double *transform_out, double *mean_out, double *llk_in);
/* ppca_heldout_score under known precisions.  (z, Sigma) is the posterior of row i given its entries in `train` under
 * the precisions `train_prec` (ppca_h_estep's; a row without an observed train entry has z = 0, Sigma = I).  Every entry of `held`
 * that is observed under `held_prec` (x finite, q finite and > 0) is scored as a new reading of column j:
 *   m = mean_j + c_j . z,  v = sigma^2 / q_ij + c_j^T Sigma c_j,  e = x - m,  l = -1/2 (ln 2 pi + ln v + e^2 / v)
 * held_prec may be the handle train_prec (the usual case after ppca_dataset_holdout of x: whether an entry is observed follows x).  A
 * held precision < 0 or = +inf at a finite x is PPCA_ERR_INVALID with no output written; bad train precisions are reported as
 * ppca_h_estep reports them.  Outputs, weights and the reproducibility contract are ppca_heldout_score's (per_row depends on its row
 * alone; PPCA_HELD_CHUNK forces a chunk length); no N x d buffer is allocated.  Covers 1 <= k <= 16 and 1 <= d <= 1024. */
int ppca_h_heldout_score(ppca_ctx *ctx, ppca_dataset *train, ppca_dataset *train_prec, ppca_dataset *held, ppca_dataset *held_prec,
                         const ppca_model *model, double *totals_host, double *col_sums_host, double *per_row);

/* --------------------------------------------------- masked PPCA on row-compressed data */
/* An extension with no reference counterpart: the dataset as CSR -- row_ptr (int64, n + 1, monotone from 0 to nnz), col (int32, nnz,
 * strictly increasing within a row, in [0, d)), val (fp64, nnz, finite) -- for data of which 0.1-3 % exists (ratings, assays), where
 * the n x d form of ppca_dataset does not fit or is mostly NaN.  An entry that is absent is masked.  The model, the packed statistics
 * (ppca_stats_len) and the M-step are the dense path's: ppca_sparse_em_accumulate produces the same additive buffer from a row pass
 * over the CSR and a column pass over an inverted index that the constructor builds on the host.  State sizes 0 .. 16 (0 as one zero
 * column; more: PPCA_ERR_UNSUPPORTED before any launch), any d >= 1; an empty dataset (n = 0): PPCA_ERR_EMPTY from every compute entry.
 *
 * Rows are processed in blocks of block_rows, a long column of a block in runs of `segment` entries (0 = the defaults: the records of
 * a block stay under 1 GiB at k = 16; 512 entries).  The log-density, posterior mean and covariance of a row depend on its entry list
 * alone: bit-identical under any grid limit, block_rows, weights or position.  For a given (block_rows, segment) the whole statistics
 * buffer is bit-reproducible under any grid limit (fixed-order sums, no float atomics).  Hold-out splits and held-out scores of such
 * data: ppca_heldout_split_csr_host and ppca_heldout_score_sparse, at the end of this section. */
typedef struct ppca_sparse ppca_sparse;
/* Any violation of the format above is PPCA_ERR_INVALID before any device work.  weights: n or NULL (= 1). */
int ppca_sparse_from_host(ppca_ctx *ctx, int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val,
                          const double *weights, int64_t block_rows, int32_t segment, ppca_sparse **out);
/* The inverted index on host buffers (no GPU needed): per block of block_rows rows (0 = the default) a counting sort of the block's
 * entries by column, stable in row order.  Block b covers the entries [row_ptr[b block_rows], row_ptr[min(n, (b + 1) block_rows)]) and
 * writes that range of t_row_out (int32: the row within the block) and t_val_out; col_ptr_out (nullable, blocks x (d + 1)): the column
 * offsets relative to the block's first entry.  Validates like the constructor, which calls the same routine. */
int ppca_sparse_transpose_host(int64_t n, int32_t d, const int64_t *row_ptr, const int32_t *col, const double *val, int64_t block_rows,
                               int64_t *col_ptr_out, int32_t *t_row_out, double *t_val_out);
/* ppca_sparse_from_host for CSR arrays that already live on the device.  The three arrays and the weights (n or NULL)
 * are borrowed the way ppca_dataset_from_device borrows x: the library never writes or frees them and the caller keeps them alive as
 * long as the handle, or any handle made from it, lives.  The format is validated on the device by the rules above; a violation is
 * PPCA_ERR_INVALID before anything is built, and the message names the lowest offending row whatever the grid.  The row lists, the
 * inverted index and the work items are built on the device and equal those of ppca_sparse_from_host on the same arrays, integer for
 * integer (t_val: the input's bits), so every pass gives the same bits on either handle.  A few integers per block and one flag per
 * column come back to the host; nothing of size nnz does.  ppca_sparse_build_seconds: the wall time of the build, its waits included. */
int ppca_from_device_sparse(int64_t n, int32_t d, ppca_ctx *ctx, const int64_t *row_ptr_dev, const int32_t *col_dev, const double *val_dev,
                            const double *weights_dev, int64_t block_rows, int32_t segment, ppca_sparse **out);
/* The index of a handle from either constructor, block by block (0 <= block < *n_blocks_out of ppca_n_blocks_sparse), every output
 * nullable:
 *   counts_out   (13) row0, rows, e0, nnz, nbin[3], bin_off[3], n_items, n_long, n_runs of the block
 *   col_ptr_out  (d + 1) the block's column offsets relative to e0, recomputed from the items
 *   t_row_out    (nnz of the block, int32) and t_val_out (fp64; a values view: the view's): the inverted index
 *   rowlist_out  (rows, int32) the three row lists end to end
 *   items_out    (n_items x 24 bytes: int64 start, int64 dest, int32 col, int32 len) and longs_out (n_long x 16 bytes: int64 first,
 *                int32 col, int32 nruns): the work items of the column pass
 * block = -1: counts_out = n, nnz, block_rows, segment, max_rows, max_runs, nonempty_rows, d, n_blocks, 0 .. (no other output). */
int ppca_index_to_host_sparse(int64_t block, ppca_sparse *sp, int64_t *counts_out, int64_t *col_ptr_out, int32_t *t_row_out, double *t_val_out,
                              int32_t *rowlist_out, void *items_out, void *longs_out);
int ppca_n_blocks_sparse(int64_t *n_blocks_out, const ppca_sparse *sp);
int ppca_sparse_free(ppca_sparse *sp);
int64_t ppca_sparse_len(const ppca_sparse *sp);
int32_t ppca_sparse_output_size(const ppca_sparse *sp);
int64_t ppca_sparse_nnz(const ppca_sparse *sp);
double ppca_sparse_build_seconds(const ppca_sparse *sp); /* host time the constructor spent on the index, row lists and work items */
/* Shares the entries and the index; weights_host: n or NULL (= 1). */
int ppca_sparse_with_weights(ppca_sparse *sp, const double *weights_host, ppca_sparse **out);
/* The CSR arrays and the weights back (each nullable). */
int ppca_sparse_to_host(ppca_sparse *sp, int64_t *row_ptr, int32_t *col, double *val, double *weights);
/* flags[j] = 1 iff column j has no entry (from the column counts of the index; no device work). */
int ppca_sparse_empty_dimensions(ppca_sparse *sp, int32_t *flags);
/* ppca_em_accumulate / ppca_em_step / ppca_stats_raw / ppca_llk / ppca_infer on row-compressed data.  ppca_sparse_em_step leaves its
 * log-likelihood for ppca_em_last_llk like ppca_em_step.  An empty row has ell = 0, z = 0, Sigma = I. */
int ppca_sparse_em_accumulate(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *stats_dev);
int ppca_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model_in, const ppca_prior *prior, ppca_model *out,
                        double *llk_in);
int ppca_sparse_stats_raw(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *stats_host);
int ppca_sparse_llk(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *total_host, double *per_row_host);
int ppca_sparse_infer(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double *states_host, double *covs_host);
/* The predictive of a NEW reading at the query positions (query_row_ptr: n + 1, monotone from 0; query_col in [0, d), any order), given
 * each row's entries in sp: mean = mean_j + c_j . z_i, var = c_j^T Sigma_i c_j + sigma^2 (the convention of ppca_heldout_score), one
 * value per query entry in query order.  No n x d buffer exists anywhere. */
int ppca_sparse_predict(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, const int64_t *query_row_ptr, const int32_t *query_col,
                        double *mean_host, double *var_host);
/* The n_top best columns of every row: the score of column j for row i is mean + kappa sqrt(var) with ppca_sparse_predict's
 * (mean, var) of position (i, j), evaluated fma(kappa, sqrt(var), mean); kappa = 0 ranks by the mean and reads no covariance.  Ranked
 * are the candidate columns (candidates: n_candidates strictly increasing columns in [0, d), or NULL = all d) -- with exclude_observed
 * != 0 those of them the row has no entry in -- by score descending, equal scores by ascending column; a score that is NaN or -inf
 * is not ranked.  cols_host (int32, n x n_top) and scores_host (fp64, n x n_top), host memory: the row's list, padded at the end with
 * -1 and NaN where it has fewer than n_top candidates.  Row weights play no part; an empty row ranks with z = 0, Sigma = I; state size 0
 * runs as one zero column (the score is mean_j).  The scores are ppca_sparse_predict's bit for bit and the order is total: the result
 * is bit-identical under any grid limit and block_rows.  No n x d buffer and no float atomics.
 * Preconditions, all checked before any device work: 1 <= n_top <= 64, kappa finite, candidates as above (else PPCA_ERR_INVALID);
 * k <= 16 (else PPCA_ERR_UNSUPPORTED); n = 0: PPCA_ERR_EMPTY.  (Named with the family first, like ppca_heldout_score_sparse.) */
int ppca_topn_sparse(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, int32_t n_top, double kappa, int32_t exclude_observed,
                     const int32_t *candidates, int64_t n_candidates, int32_t *cols_host, double *scores_host);
/* The mixture (ppca_mix_*) on row-compressed data: n_models components of sp's output size, any state sizes <= 16
 * (state size 0 as one zero column), any number of them.  ell_c of a row is ppca_sparse_llk's of component c alone, bit for bit: one
 * row pass computes it for all components of a state size, the row's entries read once.
 * ppca_mix_sparse_llk: ppca_mix_llk -- per_row_host (n) the mixture log-density of each row, total_host its sum under sp's weights,
 * log_posteriors_host (n x n_models) the log posterior over the components; each output nullable.  An empty row has ell_c = 0 for
 * every c: its posterior is the prior weights.
 * ppca_mix_sparse_component_llks: out_host (n_models x n, component-major) = the ell_c behind the above (for tests and diagnostics).
 * ppca_mix_sparse_em_step: ppca_mix_em_step -- the same sequence, output-aliasing checks and priors, a row of weight <= 0 contributes
 * nothing; everything is enqueued on the context stream and the n_models + 1 returned numbers are read back behind one synchronisation
 * (a mean prior adds its host solve per component).  Where the dense step drops the rows whose weight is below 2^-200 of the
 * component's largest from that component's pass, this one does not gather rows (the row lists and the inverted index are fixed): such
 * rows enter with their negligible weight, and the two agree to far below fp64 resolution.
 * ppca_mix_sparse_predict: ppca_sparse_predict for the mixture.  With r_c the row's posterior given its entries in sp and (m_c, v_c)
 * ppca_sparse_predict's pair under component c: mean = sum_c r_c m_c, var = sum_c r_c v_c + sum_c r_c (m_c - mean)^2, the components
 * added in index order by the one thread that owns the query entry: bit-identical under any grid limit and block_rows.  The scratch is
 * one block's states and covariances of ONE component and n_models means per query entry of the block; no n x d buffer, no float
 * atomics.
 * Preconditions of all four, checked before any device work: n_models >= 1, every model of sp's d and on sp's device (else
 * PPCA_ERR_INVALID); every k <= 16 (else PPCA_ERR_UNSUPPORTED); n = 0: PPCA_ERR_EMPTY.  (Named with the family first, like
 * ppca_topn_sparse.) */
int ppca_mix_sparse_llk(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                        double *total_host, double *per_row_host, double *log_posteriors_host);
int ppca_mix_sparse_component_llks(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, int32_t n_models, double *out_host);
int ppca_mix_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models_in, const double *log_weights_in, int32_t n_models,
                            const ppca_prior *prior, ppca_model *const *models_out, double *log_weights_out, double *llk_in);
int ppca_mix_sparse_predict(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                            const int64_t *query_row_ptr, const int32_t *query_col, double *mean_host, double *var_host);
/* ppca_topn_sparse for the mixture: the n_top best columns of every row under n_models components (as above: sp's
 * output size, any state sizes <= 16, state size 0 as one zero column, any number of them).  The score of column j for row i is
 * fma(kappa, sqrt(var), mean) with ppca_mix_sparse_predict's (mean, var) of position (i, j), bit for bit: with r_c = exp(log posterior
 * of component c given the row's entries) and (m_c, v_c) ppca_sparse_predict's pair under component c, mean = r_0 m_0, then
 * fma(r_c, m_c, mean) in index order; var likewise from the v_c; then var + s with s = fma(r_c, (m_c - mean)^2, s) from 0 in index
 * order.  kappa = 0 ranks by the mean and forms or reads no covariance.  Candidates, exclude_observed, the order (score descending,
 * equal scores by ascending column; NaN and -inf are not ranked), the outputs and their padding with -1 / NaN are ppca_topn_sparse's.
 * Row weights play no part; an empty row ranks under the prior weights with z = 0, Sigma = I per component; a one-component mixture
 * gives ppca_topn_sparse's columns and score bits.  The scratch is one block's states (and, with kappa != 0, covariances) of ALL
 * components in the layout of the largest state size, and one weight per (row, component); no n x d buffer, no float atomics,
 * bit-identical under any grid limit and block_rows.
 * Preconditions, all checked before any device work: those of the four calls above, then 1 <= n_top <= 64, kappa finite, non-null
 * outputs, candidates strictly increasing in [0, d) (else PPCA_ERR_INVALID).  (Named with the family first, like ppca_topn_sparse.) */
int ppca_mix_topn_sparse(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t n_models,
                         int32_t n_top, double kappa, int32_t exclude_observed, const int32_t *candidates, int64_t n_candidates,
                         int32_t *cols_host, double *scores_host);
/* The hold-out split of ppca_dataset_holdout_range on the pattern of row-compressed data, on host buffers (no GPU needed; DESIGN.md
 * 4.21).  row_ptr (n + 1, from 0, monotone) and col (>= 0) as above.  Entry e of row i, column j = col[e], global row
 * g = row_offset + i draws the word of the dense split, u = (row_word(row_key(seed, 8, g), j) >> 11) 2^-53, and
 * held_flag_out[e] = 1 iff lo <= u < hi, else 0: the entries held are exactly those the dense split holds in the same matrix.
 * counts_out (nullable, 2) = [entries kept, entries held].  Requires 0 <= lo <= hi <= 1 (anything else, or NaN), row_offset >= 0 and a
 * monotone row_ptr, else PPCA_ERR_INVALID. */
int ppca_heldout_split_csr_host(int64_t n, const int64_t *row_ptr, const int32_t *col, double lo, double hi, uint64_t seed,
                                int64_t row_offset, uint8_t *held_flag_out, int64_t *counts_out);
/* The same split on the device: the entries of sp that ppca_heldout_split_csr_host flags go to *held_out, the others to
 * *train_out, both new handles with device-owned CSR arrays (columns and value bits kept, in order), sp's block_rows, segment and
 * weights (shared, not copied), their index built as by ppca_from_device_sparse.  A values view is split by its own values.
 * counts_out (nullable, 2) = [entries kept, entries held].  Preconditions and codes of the host routine; free both with
 * ppca_sparse_free, in any order with sp. */
int ppca_heldout_split_sparse(double lo, double hi, uint64_t seed, int64_t row_offset, ppca_ctx *ctx, ppca_sparse *sp,
                              ppca_sparse **train_out, ppca_sparse **held_out, int64_t *counts_out);
/* ppca_heldout_score on row-compressed data: (z, Sigma) is the posterior of row i given its entries in `train`
 * (ppca_sparse_infer; an empty row: 0, I) and every entry x of `held` in that row is scored as a new reading of column j,
 *   m = mean_j + c_j^T z,  v = sigma^2 + c_j^T Sigma c_j,  e = x - m,  l = -1/2 (ln 2 pi + ln v + e^2 / v)
 * whatever `train` has at j.  Weights are train's; held's are ignored.  Outputs as ppca_heldout_score (all host memory): per_row
 * (nullable, n) = sum_j l, 0 for a row without held entries; col_sums_host (nullable, 4 d) = per column [sum w, sum w l, sum w e^2,
 * sum w e^2 / v]; totals_host (6) = those four added over the columns in index order, the unweighted entry count, the rows with a
 * held entry.  A `held` without entries gives zeros.  State size 0 runs as one zero column: (mean_j, sigma^2).
 * Preconditions: k <= 16 (else PPCA_ERR_UNSUPPORTED before any launch); equal n, d, device and block_rows of the two datasets (else
 * PPCA_ERR_INVALID: block b of each must cover the same rows); n = 0: PPCA_ERR_EMPTY.
 * No n x d buffer and no float atomics; the scratch is one block's states and covariances.  per_row[i] depends on the row's train
 * and held entry lists alone: bit-identical under any grid limit, block_rows, weights or position.  For a given (block_rows,
 * segment) of `held` the column sums are bit-identical under any grid limit. */
int ppca_heldout_score_sparse(ppca_ctx *ctx, ppca_sparse *train, ppca_sparse *held, const ppca_model *model, double *totals_host,
                              double *col_sums_host, double *per_row);
/* Factor analysis (per-column noise, section "factor analysis" above) on row-compressed data.
 * ppca_scale_columns_sparse: ppca_dataset_scale_columns on the entries of sp, on the device, with per-column host vectors a, b, l (d
 * each; b, l nullable = 0; every element finite, else PPCA_ERR_INVALID before any device work):
 *   out     (nullable) a values view of sp: a ppca_sparse that shares sp's pattern, row lists, inverted index and work items (nothing
 *           is re-indexed) and carries sp's weights, with buffers of its own for the values val_e a_col(e) -- one fp64 multiply -- in CSR
 *           order and in index order (16 bytes per entry; the two copies of an entry hold the same bits).  Every entry point that takes
 *           a ppca_sparse takes a view, ppca_sparse_to_host returns the view's own values, ppca_sparse_free releases its two buffers to
 *           the context's block cache.  With out == NULL no per-entry buffer is allocated.
 *   col_sums_host (nullable, 3 d): tot_j = sum w_i | sum_j = sum w_i (x_ij a_j - b_j) | sq_j = sum w_i (x_ij a_j - b_j)^2 over the
 *           entries of column j, w = sp's weights; zeros for a column without an entry
 *   row_sums_host (nullable, n, host memory): sum of l_j over the row's entries; 0 for an empty row
 * At least one output is given.  The row sums and the values depend on the row's entry list alone: bit-identical under any grid limit,
 * block_rows, weights or position.  The column sums are added in a fixed order (chunks of 16 entries by a butterfly, chunks in order,
 * runs in run order, blocks in order; no float atomics): bit-identical under any grid limit for a given (block_rows, segment).  An
 * empty dataset gives zeros and a view without entries.  Synchronises once.
 * ppca_fa_sparse_em_step: ppca_fa_em_step on row-compressed data -- whiten and take sq in one scale pass (a = 1 / s, b = mean / s), the
 * row and column passes of ppca_sparse_em_accumulate on the view under PPCAModel(1, C / s, mean / s), the statistics to the host and
 * ppca_fa_finalize_host unchanged; the view is released before returning.  llk_in (nullable): the pass's by-product minus
 * sum_j tot_j ln s_j.  One synchronisation for the results (the upload of the whitened model waits once before it).  Preconditions,
 * checked before any launch: sp's d equals d (else PPCA_ERR_INVALID); k <= 16 (else PPCA_ERR_UNSUPPORTED); n = 0: PPCA_ERR_EMPTY; noise
 * positive and finite. */
int ppca_scale_columns_sparse(ppca_ctx *ctx, ppca_sparse *sp, const double *a_host, const double *b_host, const double *l_host,
                              ppca_sparse **out, double *col_sums_host, double *row_sums_host);
int ppca_fa_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, int32_t d, int32_t k, const double *noise, const double *transform,
                           const double *mean, const double *min_noise, double *noise_out, double *transform_out, double *mean_out,
                           double *llk_in);
/* Student-t PPCA (section "Student-t PPCA" above) on row-compressed data: state sizes 1 .. 16 and ANY output size
 * (the limit of 1024 above is the dense sweep's register budget, not the model's).
 * ppca_t_sparse_estep: ppca_t_estep on the entries of sp.  Per block the row pass of ppca_sparse_infer / ppca_sparse_llk writes z and the
 * Gaussian log-density of every row to scratch, one row kernel forms delta, u, ell from them, and one kernel over the inverted index
 * takes the column sums.  Every output is nullable; at least one must be given (all host memory).
 *   scaled_out     a values view of sp (ppca_scale_columns_sparse): fl(fl(sqrt(u_i)) fl(x_ij - mean_j)) in CSR order and in index order
 *                  (16 bytes per entry; the two copies of an entry hold the same bits), on sp's pattern, index and weights; without it
 *                  no per-entry buffer is allocated
 *   col_sums_host, u_host, maha_host, llks_host, scalars_host   ppca_t_estep's, with m_ij = 1 on the entries of sp; the third scalar
 *                  sums over every row, an empty one (u = 1: g[0] - 1) included
 * u, delta, ell and the view depend on the row's entry list alone: bit-identical under any grid limit, block_rows, segment, weights or
 * position.  Sums and scalars are added in a fixed order (entries of a work item in ascending row, runs in run order, blocks in order;
 * 1024 rows per workgroup in a fixed tree; no float atomics): bit-identical under any grid limit for a given (block_rows, segment); a
 * column without an entry gives zeros.  An empty dataset gives zeros and a view without entries.  Synchronises once.
 * ppca_t_sparse_em_step: ppca_t_em_step on row-compressed data -- (sigma, C, mean), (sigma, C, 0) and the tables uploaded without a
 * wait, the E-step with the view and the sums, the row and column passes of ppca_sparse_em_accumulate on the view under (sigma, C, 0),
 * statistics and sums to the host and ppca_t_finalize_host unchanged; the view is released before returning.  llk_in, q_out as
 * ppca_t_em_step.  One synchronisation of its own.
 * Preconditions, checked before any device work: sp's d equals the model's, dof positive and finite, an output given (else
 * PPCA_ERR_INVALID); 1 <= k <= 16 (else PPCA_ERR_UNSUPPORTED); the step on n = 0: PPCA_ERR_EMPTY. */
int ppca_t_sparse_estep(ppca_ctx *ctx, ppca_sparse *sp, const ppca_model *model, double dof, ppca_sparse **scaled_out,
                        double *col_sums_host, double *u_host, double *maha_host, double *llks_host, double *scalars_host);
int ppca_t_sparse_em_step(ppca_ctx *ctx, ppca_sparse *sp, int32_t d, int32_t k, double sigma, const double *transform,
                          const double *mean, double dof, double *sigma_out, double *transform_out, double *mean_out, double *llk_in,
                          double *q_out);
/* PPCA with a known precision per entry (section "PPCA with a known precision per entry" above) on row-compressed data (DESIGN.md
 * 4.30): state sizes 1 .. 16 and ANY output size (the limit of 1024 above is the dense sweep's).  An entry is observed iff it is
 * stored, and every stored entry has a precision that is finite and > 0 -- unlike the dense rule there is NO masking precision here
 * (p = 0 or NaN): an entry that should not count is not stored.  Per row and per column the quantities are those of ppca_h_estep with
 * O the row's stored entries; an empty row has ell = 0, z = 0, Sigma = I.
 * ppca_h_sparse_precisions: the precisions of sp's entries as a values view of sp (ppca_scale_columns_sparse's: it shares sp's
 * pattern, row lists, inverted index, work items and weights; 16 bytes per entry of its own).  prec_host: nnz doubles in the order of
 * sp's values (CSR), each finite and > 0, else PPCA_ERR_INVALID before any device work.  The CSR-order copy is uploaded; the
 * index-order copy is filled on the device (per index entry, a bisection of its row's column list).  Synchronises once.  Release
 * with ppca_sparse_free.
 * The three passes take (sp, prec) with prec a view made from sp or from a dataset that shares sp's pattern on the device
 * (ppca_sparse_with_weights); anything else is PPCA_ERR_INVALID: no pattern is compared on the device.
 * ppca_h_sparse_estep: ppca_h_estep's outputs and nullability (llks n, states n x k, covs n x k x k: host or device destinations;
 * stats_host: ppca_h_stats_len(d, k) doubles in ppca_h_estep's layout and order; scalars_host: 4 doubles, sum w | sum w ell | rows
 * with an entry | 0).  ell, z and Sigma of a row depend on its entry list alone: bit-identical under any grid limit, block_rows,
 * segment, weights or position.  The statistics are added in a fixed order (entries of a work item in ascending row, runs in run
 * order, blocks in order; no float atomics): bit-identical under any grid limit for a given (block_rows, segment).  They live in
 * scratch of the pass's own: ppca_em_last_llk keeps reporting the last plain step.
 * ppca_h_sparse_em_step: ppca_h_em_step on row-compressed data -- model upload, E-step, one wait for the results, then the M-step of
 * ppca_h_finalize_host (the same code, without that entry's limit on d).  llk_in (nullable): sum_i w_i ell_i of the INPUT model.
 * ppca_h_sparse_predict: ppca_sparse_predict under the posterior of the known-precision model: mean = mean_j + c_j . z and
 * var = c_j^T Sigma c_j + sigma^2, the predictive of a reading at UNIT precision (one at precision q has var + sigma^2 (1 / q - 1)); a
 * row without an entry gives the prior predictive (mean_j, |c_j|^2 + sigma^2).
 * Preconditions of the three, checked before any device work: sp's d equals the model's, prec a view of sp (else PPCA_ERR_INVALID);
 * 1 <= k <= 16 (else PPCA_ERR_UNSUPPORTED); n = 0: PPCA_ERR_EMPTY.  (The model or the host arrays lead the parameter lists, as in
 * ppca_model_download and the *_finalize_host family.) */
int ppca_h_sparse_precisions(const double *prec_host, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse **view_out);
int ppca_h_sparse_estep(const ppca_model *model, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse *prec, double *llks, double *states,
                        double *covs, double *stats_host, double *scalars_host);
int ppca_h_sparse_em_step(int32_t d, int32_t k, double sigma, const double *transform, const double *mean, ppca_ctx *ctx, ppca_sparse *sp,
                          ppca_sparse *prec, double *sigma_out, double *transform_out, double *mean_out, double *llk_in);
int ppca_h_sparse_predict(const ppca_model *model, ppca_ctx *ctx, ppca_sparse *sp, ppca_sparse *prec, const int64_t *query_row_ptr,
                          const int32_t *query_col, double *mean_host, double *var_host);

/* ------------------------------------------- sample-sharded EM across GPUs */
/* The dataset shards by contiguous row blocks (the rule of Dataset.chunks, src/python_bindings.rs:110-118); every
 * statistic above is a weighted sum over samples, so ONE all-reduce(sum) of the packed buffer per iteration
 * replaces the reference's in-process rayon reductions (ppca_model.rs:290-293, :350-358), and every rank finalises
 * the same model.  The collective is RCCL (resolved at run time with dlopen) on the context stream.
 *
 * One process (or thread) per GPU:  rank 0 calls ppca_comm_unique_id, the host ships the 128 bytes to the other
 * ranks by its own means (MPI, a file, torch.distributed's store), every rank calls ppca_comm_create -- a
 * collective call.  One thread driving several GPUs: ppca_comm_create_all + ppca_em_step_group. */
typedef struct ppca_comm ppca_comm;
#define PPCA_UNIQUE_ID_BYTES 128
int ppca_comm_unique_id(void *id_out /* PPCA_UNIQUE_ID_BYTES */);
int ppca_comm_create(ppca_ctx *ctx, int32_t n_ranks, int32_t rank, const void *unique_id, ppca_comm **out);
/* n contexts on n distinct devices of this process -> n communicators (out[n]) of one clique. */
int ppca_comm_create_all(ppca_ctx *const *ctxs, int32_t n, ppca_comm **out);
int ppca_comm_destroy(ppca_comm *comm);
int32_t ppca_comm_n_ranks(const ppca_comm *comm);
int32_t ppca_comm_rank(const ppca_comm *comm);
/* "rccl <version> via <library>" or "unavailable: <why>". */
const char *ppca_comm_backend(void);
/* In-place all-reduce of n doubles of device memory over the ranks, on the context stream (asynchronous).
 * op 0 = sum, 1 = max (the mixture's per-component maxima, mix.rs:312-317). */
int ppca_comm_allreduce(ppca_comm *comm, double *buf_dev, int64_t n, int32_t op);
/* PPCAModel::iterate_with_prior (ppca_model.rs:277-393) over ALL shards: this rank's ppca_em_accumulate, the
 * all-reduce, ppca_em_finalize -- enqueued back to back on the context stream, no host synchronisation unless
 * llk_in (log-likelihood of model_in over all shards) is requested.  A rank whose shard is empty still calls. */
int ppca_em_step_sharded(ppca_comm *comm, ppca_dataset *shard, const ppca_model *model_in, const ppca_prior *prior,
                         ppca_model *out, double *llk_in);
/* The same from ONE host thread for the n communicators of ppca_comm_create_all (shards[i], models_in[i],
 * models_out[i] live on comms[i]'s device; the all-reduces are issued as one RCCL group). */
int ppca_em_step_group(ppca_comm *const *comms, int32_t n, ppca_dataset *const *shards, ppca_model *const *models_in,
                       const ppca_prior *prior, ppca_model *const *models_out, double *llk_in);

/* PPCAMix::iterate_with_prior (mix.rs:281-337) over ALL row shards in ONE call per rank (BASELINE configuration 5):
 * this rank's responsibilities (K log-likelihood sweeps), an all-reduce(MAX) of the K per-component maxima of
 * ln w_i + log r_ic (:312-317 take them over all samples), the K weighted component passes (rows of negligible weight
 * dropped, see ppca_mix_component_stats), ONE all-reduce(SUM) of [K statistic buffers | K weight sums | llk], and the
 * identical finalisation and new log-weights (:324-325, :335) on every rank -- everything enqueued on the context
 * stream, the shifts computed on the device, one synchronisation at the end for the (K + 1) returned values.
 * models_in / models_out: n_models handles on the communicator's device (state sizes may differ per component);
 * llk_in (nullable): mixture log-likelihood of the input over all shards.  A rank whose shard is empty still calls. */
int ppca_mix_em_step_sharded(ppca_comm *comm, ppca_dataset *shard, ppca_model *const *models_in,
                             const double *log_weights_in, int32_t n_models, const ppca_prior *prior,
                             ppca_model *const *models_out, double *log_weights_out, double *llk_in);

/* Rows of this context's shard that each component pass of the most recent ppca_mix_em_step / ppca_mix_em_step_sharded
 * gathered (the others carried a weight below 2^-200 of the component's largest, see ppca_mix_component_stats): what the
 * step EXECUTED, for measurement (bench.py --config 5). */
int ppca_mix_last_rows_used(ppca_ctx *ctx, int64_t *rows, int32_t n_models);

/* ---------------------------------------------------------------- mixture */
/* PPCAMix::iterate_with_prior mix.rs:281-337 on one GPU: per-sample
 * responsibilities (log-softmax of llk_c + log pi_c, :283-295), per-component
 * weighted EM step (:297-330), new log-weights (:335).  models_in/out: n_models
 * handles of one output size d; state sizes may differ per component (mix.rs:50-71).  llk_in (nullable): mixture log-likelihood of the input
 * (PPCAMix::llk :162-174).  Samples with weight <= 0 contribute nothing
 * (documented divergence from :304-309/:326). */
int ppca_mix_em_step(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models_in, const double *log_weights_in,
                     int32_t n_models, const ppca_prior *prior, ppca_model *const *models_out,
                     double *log_weights_out, double *llk_in);
/* PPCAMix::llks :152-159 / llk :162-174 / infer_cluster :179-189 (log posteriors n x n_models). */
int ppca_mix_llk(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models, const double *log_weights,
                 int32_t n_models, double *total_host, double *per_sample_host, double *log_posteriors_host);

/* Building blocks of the sample-SHARDED mixture step (one process per GPU; the caller owns the collectives):
 * ppca_mix_responsibilities_dev: u[c][i] = ln w_i + log r_ic (mix.rs:283-309; -inf for w_i <= 0) into u_dev
 *   (n_models x n, component-major) and the per-sample mixture llk (:137-149) into lse_dev (nullable);
 * ppca_vector_max_dev: max_i v_i skipping NaNs (:312-317); ppca_vector_exp_shift_dev: out_i = exp(v_i - shift)
 *   (:320-323) -- the per-component sample weights once the maximum over ALL shards is known;
 * ppca_vector_sum_dev: sum_i v_i (w_i) (:324-325 and the llk total). */
int ppca_mix_responsibilities_dev(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models, const double *log_weights,
                                  int32_t n_models, double *u_dev, double *lse_dev);
/* One component of the sharded M-step in one call: weights exp(u_i - shift) (mix.rs:320-323; shift = the maximum over
 * ALL shards), their sum over this shard (nullable), and the component's weighted statistics (ppca_stats_len doubles,
 * device).  Every statistic is linear in the weights, so rows whose weight is below 2^-200 of the component's largest
 * (their terms sit >= 147 binary orders below the fp64 resolution of the sums they would join) are dropped: the pass
 * gathers the others (rows_used, nullable, reports how many).  Synchronises. */
int ppca_mix_component_stats(ppca_ctx *ctx, ppca_dataset *ds, const ppca_model *model, const double *u_dev, double shift,
                             double *stats_dev, double *sum_host, int64_t *rows_used);
int ppca_vector_max_dev(ppca_ctx *ctx, const double *v_dev, int64_t n, double *max_host);
int ppca_vector_exp_shift_dev(ppca_ctx *ctx, const double *v_dev, double shift, int64_t n, double *out_dev);
int ppca_vector_sum_dev(ppca_ctx *ctx, const double *v_dev, const double *w_dev, int64_t n, double *sum_host);

/* PPCAMix::smooth / extrapolate (mix.rs:245-265, through InferredMaskedMix::smoothed :404-412 and
 * ::extrapolated :414-423) and the diagonal covariances around the mixture mean
 * (smoothed_covariance_diagonal :447-461, extrapolated_covariance_diagonal :489-505): posterior-weighted
 * sums over the components.  mode 0 smooth, 1 extrapolate, 2 smoothed covariance diagonal,
 * 3 extrapolated covariance diagonal.  The output dataset carries no weights (the reference collects
 * fresh samples). */
int ppca_mix_reconstruct(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models, const double *log_weights,
                         int32_t n_models, int32_t mode, ppca_dataset **out);

/* PosteriorSamplerMix (mix.rs:521-537) on the device: per row a component from its posterior (a uniform of the row's choice
 * stream against the cumulative posterior in component order), then that component's ppca_posterior_sample draw of the row
 * (component c takes the first k_c normals of the row's eps stream).  The output carries no weights. */
int ppca_mix_posterior_sample(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models, const double *log_weights,
                              int32_t n_models, int32_t mode, uint64_t seed, int64_t row_offset, ppca_dataset **out);

/* ppca_heldout_score for a mixture.  a_c = exp(lp_c), lp_c the row's log posterior of component c given `train`
 * (ppca_mix_llk); m_c, v_c, l_c the component's predictive of the held entry x as ppca_heldout_score gives it.  Per held entry
 *   l = logsumexp_c(lp_c + l_c),  A = sum_c a_c (m_c - x),  V = sum_c a_c v_c,  Q = sum_c a_c (m_c - x)^2,
 *   e = -A,  variance V + max(Q - A^2, 0)
 * (centred on x, so that the cancellation of Q - A^2 is harmless; the clamp keeps the variance >= min_c v_c).  A component of
 * weight 0 contributes nothing.  Outputs as ppca_heldout_score; a one-component mixture gives the model's result. */
int ppca_mix_heldout_score(ppca_ctx *ctx, ppca_dataset *train, ppca_dataset *held, ppca_model *const *models, const double *log_weights,
                           int32_t n_models, double *totals_host, double *col_sums_host, double *per_row);

/* The leave-one-out predictive of a mixture (an extension with no reference counterpart).  Component c gives m_cj,
 * v_cj, l_cj as ppca_loo_predictive does; lp_c is the row's log posterior of c (ppca_mix_llk).  Observed j: a_cj = exp(lp_c - l_cj - L_j)
 * with L_j = log sum_c exp(lp_c - l_cj) (the posterior of c given the row without j), l_j = -L_j.  Masked j: a_cj = exp(lp_c).  Mean
 * sum_c a_cj m_cj, variance sum_c a_cj (v_cj + (m_cj - mean_j)^2).  per_sample_host / total_host as ppca_loo_predictive (total: the
 * sample weights applied, as ppca_mix_llk).  The output datasets carry no weights, like every mixture output. */
int ppca_mix_loo_predictive(ppca_ctx *ctx, ppca_dataset *ds, ppca_model *const *models, const double *log_weights, int32_t n_models,
                            ppca_dataset **mean_out, ppca_dataset **var_out, double *total_host, double *per_sample_host);

/* ------------------------------------------------------------------ debug */
/* Test hook: cap the number of workgroups of every persistent-grid launch of this context (the fused kernels start
 * min(tiles, CUs) workgroups, each walking a contiguous run of 32-sample tiles) so that a dataset small enough for the CPU
 * oracle still gives every workgroup hundreds of tiles -- the steady state of the kernels (tile rings, software
 * pipelines, the periodic flush of the integer accumulators) under the oracle.  n_workgroups <= 0 restores the device's
 * CU count.  Results do not depend on the grid beyond the order of the partial sums. */
int ppca_ctx_set_grid_limit(ppca_ctx *ctx, int32_t n_workgroups);
/* Test hook: afterwards the context behaves as a newly created one, except that every device byte it owns or caches holds `byte`
 * (its low eight bits).  Takes the context's lock, waits for its stream, returns every scratch buffer the context keeps across calls
 * to its block cache and forgets what it remembered about them (slice tables, guard words, the place of the last log-likelihood, the
 * rows of the last mixture step, the split pipeline's trace), fills every cached block on the stream and waits again.  blocks_out /
 * bytes_out (nullable): how many blocks and bytes were filled.  Blocks that a live dataset, model or row-compressed handle owns are
 * not in the cache and are never touched; pinned host buffers stay as they are.  For tests of "no pass depends on what its recycled
 * memory held" (tests/test_gpu_recycled_memory.py); the library itself never calls it. */
int ppca_ctx_dirty_scratch(ppca_ctx *ctx, int32_t byte, int64_t *blocks_out, int64_t *bytes_out);
/* (ABI 6) Test / measurement hook of the EM pass's int8 form of the mask-side statistics (k <= 10): a 32-sample tile with at most
 * max_rows rows that do not fit the fixed-point form -- outlier samples, heavy sample weights -- sends those rows round it (exact
 * fp64 additions into the accumulators, what the reference's f64 sums do with such a row, ppca_model.rs:297-306) instead of raising
 * the exponents of its workgroup for every later row.  Default 8; 0 = the behaviour of ABI <= 5 (every such tile raises the
 * exponents; the device-side guard then repeats the affected workgroups' slices on the fp64 engine: ppca_em_last_fallback), which
 * the tests of that guard select.  Values above 32 mean 32. */
int ppca_ctx_set_heavy_rows(ppca_ctx *ctx, int32_t max_rows);
/* Diagnostic counters of the int8 statistics contraction of the EM pass on this context's device since the last reset:
 * out8[0..3] the eight-wave kernel (k <= 10), out8[4..7] the two-kernel pass (k = 11..16): [0] tiles cut again after the
 * fixed-point exponents were raised (beyond each workgroup's first tile), [1] periodic flushes of the int64
 * accumulators, [2] the largest number of tiles one workgroup walked, [3] launches.  Synchronises. */
int ppca_debug_counters(ppca_ctx *ctx, int64_t *out8, int32_t reset);

/* Test hook: what the HOST side of the split pipeline (ppca_generic.hip + ppca_solve4.hip: every shape with d > 256 or k > 16, and the
 * output passes of k = 11..16) decided in the most recent pass of this context that went through it -- which kernel variant, tile,
 * addressing form, K-split and grid each of its size-gated branches took, accumulated over the pass's chunks.  Host integers written
 * where the launches are made: no device work, no synchronisation, nothing about a launch changes.  With ppca_ctx_set_grid_limit a test
 * puts an oracle-sized dataset on the large-N side of a threshold and ASSERTS through this record that the branch ran.  Launch lists
 * keep the first PPCA_TRACE_LAUNCHES entries (the counts go on).  The fused paths (d <= 256, k <= 10; the EM pass of k = 11..16) leave it
 * alone, except that the latter marks `fused16`. */
#define PPCA_TRACE_LAUNCHES 32
typedef struct ppca_generic_trace {
    int32_t valid;    /* 0 until a pass of this context has gone through the split pipeline */
    int32_t em;       /* 1 = EM statistics pass, 0 = output pass (llk, states, covariances, reconstructions) */
    int32_t fused16;  /* 1 = an EM pass handed on to the two-kernel pass of k = 11..16, d <= 256: nothing below is filled */
    int32_t int8;     /* 1 = the int8-sliced contractions (0: PPCA_GENERIC_FP64=1 pinned the fp64 products) */
    int32_t d, k, n_cu, chunks;
    int64_t n, chunk_rows; /* rows of the pass; rows of a full chunk */
    /* int8 GEMM launches, in launch order.  role: 0 = Gram, 1 = statistics product as ONE launch (nsplit > 1: cut along the samples),
     * 2 / 3 = the statistics product as a pair: the column blocks that fill the chip, then the last ones cut along the samples */
    int32_t n_i8gemm;
    int32_t i8_role[PPCA_TRACE_LAUNCHES], i8_tile_rows[PPCA_TRACE_LAUNCHES], i8_xcd_map[PPCA_TRACE_LAUNCHES];
    int32_t i8_buffer[PPCA_TRACE_LAUNCHES]; /* 1 = buffer addressing, 0 = pointer arithmetic */
    int32_t i8_nsplit[PPCA_TRACE_LAUNCHES]; /* slices along the samples (1 = none) */
    int32_t stats_whole, stats_sliced, stats_pair; /* chunks whose statistics product took each arm */
    /* fp64 GEMM launches, in launch order.  amode: 0 Gram, 1 b = X~ C, 2 mask^T . B, 3 X~^T . B; guarded: 1 = behind a device-side
     * guard flag (runs only when the int8 form's guard tripped; the host cannot know) */
    int32_t n_gemm;
    int32_t gemm_amode[PPCA_TRACE_LAUNCHES], gemm_kslices[PPCA_TRACE_LAUNCHES], gemm_guarded[PPCA_TRACE_LAUNCHES];
    /* the one-pass form of the two skinny statistics products: launches, and of the FIRST chunk its column tiles (nt), slices along the
     * samples, blocks along the dimensions and rows per slice */
    int32_t skinny_launches, skinny_nt, skinny_slices, skinny_gy;
    int64_t skinny_rps;
    /* per-sample solver of the FIRST chunk (the largest).  solver: 1 lane, 2 lane (one wave per SIMD, k >= 13), 3 batched blocked
     * (solve4), 4 one sample per wave on the MFMA (k = 65 .. 128); 5 - 8 stood for solvers since retired and are not reused;
     * solver_nb: 16 x 16 blocks per side (3, 4) or k (1, 2); a workgroup takes solver_batch samples per iteration of its loop */
    int32_t solver, solver_nb, solver_launches;
    int64_t solver_grid, solver_batch, solver_rows;
    int32_t scal_launches, scal_blocks_max, scal_accumulated; /* scalar reduction: launches, most blocks, launches ADDING to a previous chunk's */
    int32_t wdigits_first, wdigits_predicted, wdigits_y_capped; /* chunks cut after / with their column statistics; ... whose re-cut grid was capped */
    int32_t recon_kind, recon_rpb; /* of the FIRST chunk: 0 none, 1 thread per element, 2 row-block kernel and its rows per block */
    int64_t recon_grid_x, recon_grid_y;
} ppca_generic_trace;
int ppca_generic_last_trace(ppca_ctx *ctx, ppca_generic_trace *out);

/* Which Gram engine the fused passes use for this model: 0 = int8-sliced MFMA with exact integer accumulation,
 * 1 = fp64 MFMA.  Decided on the device per model by a dynamic-range guard (the int8 form keeps 62 bits below each
 * column maximum of vech(c c^T); a model whose rows of C span many orders of magnitude, or whose sigma^2 lies
 * below that resolution, takes the fp64 form; see ppca_kernels.hip, qprep_kernel).  Stands where the reference
 * computes C_o^T C_o in f64 (output_covariance.rs:57-70).  Synchronises. */
int ppca_gram_engine(ppca_ctx *ctx, const ppca_model *model, int32_t *engine);

/* Which guards of the most recent EM pass of the fused path (d <= 256, k <= 10) on this context sent it to the fp64 engine:
 * *gram_unsafe -- the model tripped the dynamic-range guard of the int8-sliced Gram (see ppca_gram_engine);
 * *stats_unsafe -- the reduced statistics were not large against the rounding of the fixed-point form of the mask-side
 * contraction S / U / totals (a sample far above its neighbours, e.g. an outlier row, lifts its workgroup's column
 * exponents; dimensions masked in that sample then sum coarsely cut rows): the pass was repeated with fp64 accumulation,
 * as the reference sums (ppca_model.rs:297-306).  Both decided on the device; this call synchronises. */
int ppca_em_last_guard(ppca_ctx *ctx, int32_t *gram_unsafe, int32_t *stats_unsafe);

/* Bench / test hook: rows[i] of a device-resident dataset multiplied by `factor` in place (masked entries stay masked) -- how
 * `bench.py --outliers` and the guard tests put outlier samples into data generated on the device.  The dataset must own its
 * rows (not a slice or weighted view sharing another's).  Synchronises. */
int ppca_dataset_scale_rows(ppca_dataset *ds, const int64_t *rows, int64_t n_rows, double factor);

/* What the second stage of the most recent EM pass of the fused path did, decided on the device from the guards above
 * (round 5; stands where the reference's sums are plain f64, ppca_model.rs:297-306): *mode 0 = nothing; 1 = the whole pass again
 * on the fp64 engine (the model tripped the Gram guard, or too many workgroups were flagged); 2 = only the slices of the
 * *workgroups workgroups (*rows rows in all) whose fixed-point cut dominated the rounding bound -- an outlier row costs its
 * workgroup's slice, recomputed by the whole grid, not the pass.  *stage_ms (nullable): HIP-event time of the second stages
 * (fallback pass + second reduction) since timing was enabled or this was last called (0 without timing).  Synchronises. */
int ppca_em_last_fallback(ppca_ctx *ctx, int32_t *mode, int32_t *workgroups, int64_t *rows, double *stage_ms);

/* One v_mfma_f64_16x16x4_f64 on host-supplied A (16 x 4) and B (4 x 16), result
 * (16 x 16) written through the C/D lane map the kernels assume (unit test). */
int ppca_debug_mfma_probe(ppca_ctx *ctx, const double *a16x4, const double *b4x16, double *out16x16);

/* One v_mfma_i32_16x16x64_i8 on raw per-lane operand registers (a_regs, b_regs: [64 lanes][16 bytes];
 * out_regs: [64 lanes][4 i32]) -- pins the operand / result lane maps of the int8 Gram path (unit test). */
int ppca_debug_mfma_i8_probe(ppca_ctx *ctx, const int8_t *a_regs, const int8_t *b_regs, int32_t *out_regs);

#ifdef __cplusplus
}
#endif
#endif /* PPCA_HIP_H */
