// ppca_sparse_mix.hip -- the mixture on row-compressed data (ppca_mix_sparse_component_llks / _llk / _em_step / _predict; DESIGN.md
// section 4.23).  Storage and shared scaffolding: ppca_sparse.hpp.
// sparse_mix_row_kernel<K, REG>  the row pass for up to MIX_MAX components of one state size: the row's entries fetched once (REG: kept
//     in registers across the components), ell_c into the component-major buffer of launch_mix_posteriors.  Its sums, tree,
//     factorisation and ell (sp_mix_row_ell) are sparse_row_kernel's operation for operation, so ell_c is sparse_row_kernel's bit for
//     bit; sparse_row_kernel itself is left as it was.  The step is ppca_host::mix_em_step's sequence with sp_accumulate under each
//     component's weight vector.
// sparse_mix_predict_kernel, sparse_mix_spread_kernel  the mixture predictive, component by component in index order per query entry.
#include "ppca_sparse.hpp"

using namespace ppca_sp;

namespace ppca_sp {

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

// ell of one row on its group of W lanes, sparse_row_kernel's (ppca_sparse.hip) statements in sparse_row_kernel's order: each(f) calls
// f(column, value) for this lane's entries of the row in order; the lane gathers the rows of C and accumulates its own
// [G | b | |x~|^2], one butterfly of log2 W steps adds the group's lanes, then every lane factors M = sigma^2 I + G and solves.  (A
// second copy of those statements, not a helper that both kernels call: moving sparse_row_kernel's into a function changed its
// registers and schedule.  Change both.)
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

}  // namespace ppca_sp

namespace {

template <int K>
hipError_t mix_row_t(const SpMixRowArgs &a, int grid, hipStream_t s) {
    if constexpr (K < 12) {  // a lane's entries in registers: a bin where it has at most 4 of them, and a register budget with room for them
        if (a.W < 64) return sp_launch(sparse_mix_row_kernel<K, true>, grid, s, a);
    }
    return sp_launch(sparse_mix_row_kernel<K, false>, grid, s, a);
}
hipError_t launch_mix_row(int k, const SpMixRowArgs &a, int grid, hipStream_t s) { SP_DISPATCH(k, mix_row_t, a, grid, s); }

// llk[c n + i] = ell of row i under component c: the components grouped by state size, one launch of sparse_mix_row_kernel per group
// of at most MIX_MAX, block and non-empty bin
int sp_mix_rows(ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, int nm, double *llk) {
    const SpCore &c = *sp->core;
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
            a.d = c.d;
            a.nc = (int)std::min<size_t>(MIX_MAX, group.size() - g0);
            for (int i = 0; i < a.nc; ++i) {
                a.model[i] = models[group[g0 + i]]->p();
                a.llk[i] = llk + (size_t)group[g0 + i] * c.n;
            }
            const auto row = [&](const SpMixRowArgs &ba, int grid) { return launch_mix_row(k, ba, grid, ctx->stream); };
            for (const SpBlock &b : c.blocks)
                if (int rc = sp_for_bins(ctx, sp, b, a, row)) return rc;
        }
    }
    return PPCA_OK;
}

}  // namespace

int ppca_sp::sp_mix_check(const ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int32_t nm) {
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

int ppca_sp::sp_mix_blocks(ppca_ctx *ctx, int64_t n, int nm, bool want_logpost, SpMixDev *m) {
    if (int rc = ensure(ctx->mix[0], ctx->mix_cap[0], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = ensure(ctx->mix[1], ctx->mix_cap[1], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = ensure(ctx->mix[2], ctx->mix_cap[2], sizeof(double) * (size_t)n)) return rc;
    if (want_logpost)
        if (int rc = ensure(ctx->mix[3], ctx->mix_cap[3], sizeof(double) * (size_t)nm * n)) return rc;
    if (int rc = mix_aux(ctx, nm, m->ax)) return rc;
    if (int rc = ensure_hstage(ctx, sizeof(double) * m->ax.P + sizeof(int) * (size_t)nm)) return rc;
    m->llk = dptr<double>(ctx->mix[0]);
    m->u = dptr<double>(ctx->mix[1]);
    m->lse = dptr<double>(ctx->mix[2]);
    m->logpost = want_logpost ? dptr<double>(ctx->mix[3]) : nullptr;
    return PPCA_OK;
}
int ppca_sp::sp_mix_posteriors(ppca_ctx *ctx, const ppca_sparse *sp, ppca_model *const *models, const double *log_weights, int nm,
                               const SpMixDev &m) {
    if (int rc = sp_mix_rows(ctx, sp, models, nm, m.llk)) return rc;
    if (int rc = mix_upload_logw(ctx, log_weights, nm, m.ax)) return rc;
    HIP_TRY(launch_mix_posteriors(m.llk, m.ax.logw, sp->w, sp->core->n, nm, m.u, m.lse, m.logpost, ctx->stream));
    return PPCA_OK;
}

extern "C" int ppca_mix_sparse_component_llks(ppca_ctx *ctx, ppca_sparse *sp, ppca_model *const *models, int32_t n_models, double *out_host) {
    static const double none = 0.0;  // (no weights are read)
    if (!out_host) return fail(PPCA_ERR_INVALID, "null argument");
    if (int rc = sp_mix_check(ctx, sp, models, &none, n_models)) return rc;
    USE_CTX(ctx);
    const size_t len = (size_t)n_models * sp->core->n;
    if (int rc = ensure(ctx->mix[0], ctx->mix_cap[0], sizeof(double) * len)) return rc;
    if (int rc = sp_mix_rows(ctx, sp, models, n_models, dptr<double>(ctx->mix[0]))) return rc;
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
    double *work = dptr<double>(ctx->work);
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
    double *pack = dptr<double>(ctx->mixpack), *work = dptr<double>(ctx->work);
    double *aux = m.ax.shift, *wc = dptr<double>(ctx->mix[4]);
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
    BufRef stb, cvb, qp, qc, meanb, varb, cmeanb;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * kmax, &stb)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)c.max_rows * kmax * kmax, &cvb)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &meanb)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)nq, &varb)) return rc;
    if (int rc = dev_alloc(sizeof(double) * (size_t)qmax * nm, &cmeanb)) return rc;
    int rc = sp_upload(ctx, query_row_ptr, sizeof(int64_t) * (size_t)(c.n + 1), &qp);
    if (!rc) rc = sp_upload(ctx, query_col, sizeof(int32_t) * (size_t)nq, &qc);
    if (!rc) rc = sp_mix_posteriors(ctx, sp, models, log_weights, nm, m);
    const int64_t *qpd = qp ? dptr<const int64_t>(qp) : nullptr;
    const int32_t *qcd = qc ? dptr<const int32_t>(qc) : nullptr;
    double *stp = dptr<double>(stb), *cvp = dptr<double>(cvb), *cmp = dptr<double>(cmeanb), *mp = dptr<double>(meanb), *vp = dptr<double>(varb);
    for (size_t bi = 0; bi < c.blocks.size() && !rc; ++bi) {
        const SpBlock &b = c.blocks[bi];
        const int64_t q0 = query_row_ptr[b.row0], q1 = query_row_ptr[b.row0 + b.rows];
        if (q1 == q0) continue;
        const int grid = sp_elementwise_grid(q1 - q0, ctx->n_cu);
        for (int e = 0; e < nm && !rc; ++e) {  // component by component: the scratch is ONE component's states and covariances
            rc = sp_rows_of_block(ctx, sp, b, models[e], nullptr, stp, cvp, nullptr, nullptr);
            if (rc) break;
            if (sp_launch(sparse_mix_predict_kernel, grid, ctx->stream, qpd, qcd, q0, q1, b.row0, b.rows, c.d, models[e]->k, models[e]->p(), stp, cvp,
                          m.logpost, e, nm, cmp, mp, vp))
                rc = fail(PPCA_ERR_HIP, "mixture predict launch failed");
        }
        if (rc) break;
        if (sp_launch(sparse_mix_spread_kernel, grid, ctx->stream, qpd, q0, q1, b.row0, b.rows, m.logpost, nm, cmp, mp, vp))
            rc = fail(PPCA_ERR_HIP, "mixture predict launch failed");
    }
    if (!rc && hipMemcpyAsync(mean_host, mp, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    if (!rc && hipMemcpyAsync(var_host, vp, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(PPCA_ERR_HIP, "download failed");
    return sp_finish(ctx, rc, "mixture predict");  // (the uploads read the caller's buffers)
}
