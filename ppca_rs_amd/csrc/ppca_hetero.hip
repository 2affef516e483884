// ppca_hetero.hip -- the kernels behind heteroscedastic PPCA (HPPCAModel): every entry x_ij comes with a known
// precision p_ij relative to sigma^2,  x_ij = mean_j + c_j . z_i + eps_ij,  eps_ij ~ N(0, sigma^2 / p_ij).  An entry is observed iff
// x_ij is finite and p_ij is finite and > 0 (p = NaN or 0: not observed, whatever x holds; p < 0 or +inf: counted as bad, not used).
//
// For a row with observed set O (m entries), x~ = x - mean:
//     G = sum_O p c c^T    b = sum_O p x~ c    M = sigma^2 I + G    z = M^-1 b    Sigma = sigma^2 M^-1
//     ell = -1/2 [ (sum_O p x~^2 - b^T M^-1 b) / sigma^2 + ln det M + (m - k) ln sigma^2 + m ln 2 pi - sum_O ln p ],  0 when m = 0
//
// Three kernels, everything fp64 (the int8 digit tables of the Gaussian passes encode 0 / 1 masks and do not apply):
//
// hetero_sweep_kernel<K>  one read of X and P.  A wave owns 16 rows of the workgroup's 64; lane (l15, l4) takes the entries of row l15
//     at columns j0 + 4 s + l4 -- the A operand of v_mfma_f64_16x16x4 -- requested a chunk ahead with non-temporal loads (k <= 10:
//     whole lines of a row per request into a per-wave LDS tile; beyond: straight into the operand's registers).  [G | b] of the 16
//     rows is the dense contraction of the precision tile (for b: precision times x~) with the table [vech(c c^T) | C]
//     (hetero_table_kernel writes it, zero-padded to 16-column blocks; the mean rides in a padding column), staged through LDS in
//     chunks of 32 table rows (64 at k = 11, 12).  The row sums sum p x~^2, m and sum ln p (as a product of mantissas and a sum of
//     exponents: one logarithm per lane and row) are the lanes' own, added over the four column groups in a fixed order.  Then
//     [G | b] goes through LDS (the table's space) and every lane of a row factors and solves (Posterior<K>); the four lanes of a
//     row share the columns of M^-1.  Outputs per row: ell, z, optionally Sigma, and for the EM pass the record
//     R = [w z (k) | w | w (Sigma + z z^T) lower-packed], padded to 16-column blocks.
// hetero_stats_kernel<K>  the second read of X and P.  A job is a 64-column tile x a run of rows (the tiles of a run on one XCD); wave w
//     owns 16 columns.  With the
//     precisions (precision times x~) as A operand, lane <-> (column, row), and the records as B operand straight from memory:
//         (P o mask)^T R   = [V | T | S]        (P o X~)^T [w z | w] = [cross | A]
//     and sq, cnt as the lanes' own column sums from the same registers.  A job writes the partial of its own columns into
//     part[run][len]; launch_reduce_partials adds the runs in its fixed order.  No float atomics anywhere.
// hetero_recon_kernel  mean + C z everywhere (smooth), or the observed value where observed (extrapolate).
//
// ell, z and Sigma of a row depend on the row alone: the order of every sum over a row's columns is fixed by d and k (chunk by
// chunk, MFMA step by step, the lanes' groups in a fixed tree), not by the row's slot in a tile, the grid or the chunk.
#include <algorithm>

#include "ppca_device.hpp"

namespace ppca {
namespace {

typedef double d4h_t __attribute__((ext_vector_type(4)));

constexpr int H_THREADS = 256;
constexpr int H_ROWS = 64;  // rows of a workgroup step of the sweep (16 per wave)
constexpr int H_SR = 16;    // rows per loop step of the statistics kernel
constexpr int H_CT = 64;    // column tile of the statistics kernel

template <int K>
struct HCfg {
    static constexpr int KP = K * (K + 1) / 2;
    static constexpr int NG = (KP + 15) / 16;  // 16-column blocks of vech(c c^T)
    static constexpr int NT = NG + 1;          // + the block of C
    static constexpr int NTP = 16 * NT;        // table row length
    static constexpr int TS = NTP % 32 == 0 ? NTP + 16 : NTP;  // its LDS stride: the four rows a wave reads start 16 doubles apart (mod 32)
    static constexpr int GS = NTP + 1;         // [G | b] exchange stride
    static constexpr int NR = K + 1 + KP;      // record: [w z | w | w (Sigma + z z^T)]
    static constexpr int NRB = (NR + 15) / 16;
    static constexpr int NRP = 16 * NRB;
    static constexpr int NCB = (K + 1 + 15) / 16;  // the record blocks that hold [w z | w]
    static constexpr int WG_PER_CU = K <= 10 ? 2 : 1;  // k <= 10 fits 256 registers: two workgroups per CU hide each other's waits
    static constexpr int DC = (K == 11 || K == 12) ? 64 : 32;  // table rows (columns of the dataset) per staged chunk: what LDS holds
    static constexpr int XS = DC + 2;             // row stride of a wave's x / p tile: a wave half reads 16 rows x 2 columns without a conflict
    static constexpr int TILE = 2 * 16 * XS;      // a wave's tile: x then p
    static constexpr int OFF_T = DC * TS > H_ROWS * GS ? DC * TS : H_ROWS * GS;  // the table chunk, later [G | b]; behind it the four tiles
    static constexpr bool TILED = K <= 10;        // measured: the tiles win at two workgroups per CU (k = 10) and lose at one (k = 16)
    static constexpr int LDS_DOUBLES = OFF_T + (TILED ? 4 * TILE : 0);
    static_assert(LDS_DOUBLES * 8 * WG_PER_CU <= 160 * 1024, "LDS budget");
    static constexpr bool TPRE = K > 10;               // one workgroup per CU: the next table chunk waits in registers instead
    static constexpr int TPT = DC * NTP / H_THREADS;  // table doubles per thread and chunk
    static_assert(KP % 16 != 0, "column KP of the table (the padding of vech(c c^T)) holds the mean");
    static_assert(DC * NTP % H_THREADS == 0, "table chunk / threads");
};

__host__ __device__ constexpr int h_ntp(int k) { return 16 * ((k * (k + 1) / 2 + 15) / 16 + 1); }
__host__ __device__ constexpr int h_nrp(int k) { return 16 * ((k + 1 + k * (k + 1) / 2 + 15) / 16); }

// entry observed <=> x finite, p finite and > 0 (a NaN fails p > 0)
__device__ __forceinline__ bool h_observed(double x, double p) { return __builtin_isfinite(x) && p > 0.0 && p < __builtin_inf(); }
__device__ __forceinline__ bool h_bad(double p) { return p < 0.0 || p == __builtin_inf(); }

// tab[j][e]: e < kp: c_ja c_jb at e = tri(a, b); e = kp (padding of the Gram blocks: its product is never read): mean_j;
// e in [16 NG, 16 NG + k): c_j; 0 elsewhere
__global__ __launch_bounds__(256) void hetero_table_kernel(const double *model, int d, int k, double *tab) {
    const int ntp = h_ntp(k), kp = k * (k + 1) / 2, boff = ntp - 16;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)d * ntp) return;
    const int j = (int)(idx / ntp), e = (int)(idx - (int64_t)j * ntp);
    const double *c = model + MODEL_HDR + (int64_t)j * k;
    double v = 0.0;
    if (e < kp) {
        int a = 0;
        while (tri(a + 1, 0) <= e) ++a;
        v = c[a] * c[e - tri(a, 0)];
    } else if (e == kp) {
        v = model[MODEL_HDR + (int64_t)d * k + j];
    } else if (e >= boff && e < boff + k) {
        v = c[e - boff];
    }
    tab[idx] = v;
}

struct HSweepArgs {
    const double *X, *P;
    int64_t ldx, ldp, n;
    int d;
    const double *w;      // nullable (= 1)
    const double *model;  // [sigma, sigma^2, ln sigma, 0 | C | mean]
    const double *tab;    // d x NTP
    double *llks, *states, *covs, *rec;  // nullable: n | n x k | n x k x k | n x NRP
    double *scal;         // [grid][4]: sum w | sum w ell | non-empty rows | bad precisions
    int64_t rows_per_wg;  // a multiple of H_ROWS
};

template <int K>
__global__ __launch_bounds__(H_THREADS, HCfg<K>::WG_PER_CU) void hetero_sweep_kernel(HSweepArgs a) {
    using Cf = HCfg<K>;
    constexpr int H_DC = Cf::DC, NS = H_DC / 4;
    extern __shared__ double h_lds[];
    __shared__ double sred[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int d = a.d;
    const double s2 = a.model[1], lnsig = a.model[2];
    const double qnan = __builtin_nan("");
    double sw = 0.0, swl = 0.0, sne = 0.0, sbad = 0.0;
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_wg, r1 = r0 + a.rows_per_wg < a.n ? r0 + a.rows_per_wg : a.n;

    // k <= 10 (TILED): the wave's 16 x H_DC tile of X and of P for the chunk (rb, j0), requested row by row -- instruction i: row
    // i RPI + lane / H_DC of the tile, column lane % H_DC: whole lines of a row per request -- and parked in the wave's own LDS tile,
    // from which the lanes read the A operand's layout (row l15, column 4 s + l4).  NaN / 0 outside the run or past d, by selection.
    constexpr int RPI = 64 / H_DC;
    const int frow = lane / H_DC, fcol = lane % H_DC;
    double *xt_w = h_lds + Cf::OFF_T + wave * Cf::TILE, *pt_w = xt_w + 16 * Cf::XS;
    double xn[NS], pn[NS];
    auto fetch = [&](int64_t rb, int j0) {
        if constexpr (Cf::TILED) {
            const int j = j0 + fcol;
            const int jc = j < d ? j : d - 1;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int64_t r = rb + 16 * wave + i * RPI + frow;
                const bool ok = r < r1 && j < d;
                const int64_t rc = r < r1 ? r : r1 - 1;
                const double x = __builtin_nontemporal_load(a.X + rc * a.ldx + jc), p = __builtin_nontemporal_load(a.P + rc * a.ldp + jc);
                xn[i] = ok ? x : qnan;
                pn[i] = ok ? p : 0.0;
            }
        } else {  // the A operand's layout straight into registers: columns j0 + 4 s + l4 of row l15
            const int64_t r = rb + 16 * wave + l15;
            const bool live = r < r1;
            const int64_t rc = live ? r : r1 - 1;
            const double *xr = a.X + rc * a.ldx + (j0 + l4), *pr = a.P + rc * a.ldp + (j0 + l4);
            if (j0 + H_DC <= d) {  // (uniform) a whole chunk: one address per array, the columns at constant offsets
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const double x = __builtin_nontemporal_load(xr + 4 * s), p = __builtin_nontemporal_load(pr + 4 * s);
                    xn[s] = live ? x : qnan;
                    pn[s] = live ? p : 0.0;
                }
            } else {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int j = j0 + 4 * s + l4;
                    const bool ok = live && j < d;
                    const int back = j < d ? 0 : j - (d - 1);  // (the last column instead: the value is not used)
                    const double x = __builtin_nontemporal_load(xr + 4 * s - back), p = __builtin_nontemporal_load(pr + 4 * s - back);
                    xn[s] = ok ? x : qnan;
                    pn[s] = ok ? p : 0.0;
                }
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            xt_w[(i * RPI + frow) * Cf::XS + fcol] = xn[i];
            pt_w[(i * RPI + frow) * Cf::XS + fcol] = pn[i];
        }
    };
    // the table rows j0 .. j0 + H_DC (zeros past d): thread -> elements tid + 256 i of the chunk, into registers (TPRE) or LDS
    double tn[Cf::TPRE ? Cf::TPT : 1];
    auto tfetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < Cf::TPT; ++i) {
            const int e = tid + H_THREADS * i, jj = e / Cf::NTP, cc = e - jj * Cf::NTP;
            const double v = j0 + jj < d ? a.tab[(int64_t)(j0 + jj) * Cf::NTP + cc] : 0.0;
            if constexpr (Cf::TPRE)
                tn[i] = v;
            else
                h_lds[jj * Cf::TS + cc] = v;
        }
    };
    auto tstore = [&]() {
#pragma unroll
        for (int i = 0; i < Cf::TPT; ++i) {
            const int e = tid + H_THREADS * i, jj = e / Cf::NTP, cc = e - jj * Cf::NTP;
            h_lds[jj * Cf::TS + cc] = tn[i];
        }
    };
    if (r0 < r1) {
        fetch(r0, 0);
        if constexpr (Cf::TPRE) tfetch(0);
    }
    for (int64_t rb = r0; rb < r1; rb += H_ROWS) {  // (uniform over the workgroup)
        d4h_t acc[Cf::NT];
#pragma unroll
        for (int t = 0; t < Cf::NT; ++t) acc[t] = d4h_t{0, 0, 0, 0};
        double xx = 0.0, slm = 1.0;
        int sle = 0, m = 0;
        for (int j0 = 0; j0 < d; j0 += H_DC) {
            double xc[Cf::TILED ? 1 : NS], pc[Cf::TILED ? 1 : NS];
            if constexpr (Cf::TILED) {
                park();  // (the wave's own tile: its reads of the chunk before are done, LDS serves a wave in order)
            } else {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    xc[s] = xn[s];
                    pc[s] = pn[s];
                }
            }
            __syncthreads();  // the readers of the chunk before (or of [G | b] of the step before) are done
            // what the next chunk needs is requested before this chunk's products
            const bool wrap = j0 + H_DC >= d;
            const int jn = wrap ? 0 : j0 + H_DC;
            const int64_t rbn = wrap ? rb + H_ROWS : rb;
            if constexpr (Cf::TPRE) {
                tstore();
                if (rbn < r1) {
                    fetch(rbn, jn);
                    tfetch(jn);
                }
            } else {
                if (rbn < r1) fetch(rbn, jn);
                tfetch(j0);
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const double *trow = h_lds + (4 * s + l4) * Cf::TS;
                double x, p;
                if constexpr (Cf::TILED) {
                    x = xt_w[l15 * Cf::XS + 4 * s + l4];
                    p = pt_w[l15 * Cf::XS + 4 * s + l4];
                } else {
                    x = xc[s];
                    p = pc[s];
                }
                const bool o = h_observed(x, p);  // (0 where not observed, by selection: a NaN never reaches a product)
                sbad += h_bad(p) ? 1.0 : 0.0;
                const double xt = o ? __dsub_rn(x, trow[Cf::KP]) : 0.0;
                const double ap = o ? p : 0.0;
                const double apx = __dmul_rn(ap, xt);
                xx = fma(apx, xt, xx);
                m += o ? 1 : 0;
                int e = 0;
                const double f = __builtin_frexp(o ? p : 1.0, &e);
                slm *= o ? f : 1.0;
                sle += o ? e : 0;
#pragma unroll
                for (int t = 0; t < Cf::NG; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap, trow[16 * t + l15], acc[t], 0, 0, 0);
                acc[Cf::NG] = __builtin_amdgcn_mfma_f64_16x16x4f64(apx, trow[16 * Cf::NG + l15], acc[Cf::NG], 0, 0, 0);
                // (hipcc otherwise hoists every step's table reads above the first product: more registers than there are)
                if (s % 2 == 1) __builtin_amdgcn_sched_barrier(0);
            }
            {
                int e = 0;
                slm = __builtin_frexp(slm, &e);  // at most NS mantissas in [1/2, 1) since the last one: no underflow
                sle += e;
            }
        }
        __syncthreads();  // every wave has read the last chunk of the table: its space takes [G | b]
        double *gw = h_lds + (16 * wave) * Cf::GS;
#pragma unroll
        for (int t = 0; t < Cf::NT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) gw[(l4 + 4 * q) * Cf::GS + 16 * t + l15] = acc[t][q];
        __syncthreads();
        // the row's sums over its four column groups: (g0 + g1) + (g2 + g3) on every lane of the row
        double sl = log(slm) + (double)sle * LN_2;
        xx += __shfl_xor(xx, 16, 64);
        xx += __shfl_xor(xx, 32, 64);
        sl += __shfl_xor(sl, 16, 64);
        sl += __shfl_xor(sl, 32, 64);
        m += __shfl_xor(m, 16, 64);
        m += __shfl_xor(m, 32, 64);

        const double *g = gw + l15 * Cf::GS;
        Posterior<K> post;
        double pm;
        int pe;
        post.factor([&](int e) { return g[e]; }, s2, pm, pe);
        double z[K], quad, zz;
        post.solve([&](int b) { return g[16 * Cf::NG + b]; }, z, quad, zz);
        const double ell = m > 0 ? sample_llk(xx, quad, Posterior<K>::logdet(pm, pe), s2, lnsig, m, K) + 0.5 * sl : 0.0;

        const int64_t r = rb + 16 * wave + l15;
        if (r < r1) {
            const double w = a.w ? a.w[r] : 1.0;
            double *rec = a.rec ? a.rec + r * Cf::NRP : nullptr;
            if (l4 == 0) {
                if (a.llks) a.llks[r] = ell;
                if (a.states) {
#pragma unroll
                    for (int b = 0; b < K; ++b) a.states[r * K + b] = z[b];
                }
                if (rec) {
#pragma unroll
                    for (int b = 0; b < K; ++b) rec[b] = w * z[b];
                    rec[K] = w;
                }
                sw += w;
                swl = fma(w, ell, swl);
                sne += m > 0 ? 1.0 : 0.0;
            }
            if (l4 == 1 && rec) {
#pragma unroll
                for (int e = Cf::NR; e < Cf::NRP; ++e) rec[e] = 0.0;
            }
            if (a.covs || rec) {
                double *cov = a.covs ? a.covs + r * (K * K) : nullptr;
                for (int c = l4; c < K; c += 4) {  // the row's four lanes share the columns of M^-1
                    double zc = 0.0;
#pragma unroll
                    for (int b = 0; b < K; ++b) zc = b == c ? z[b] : zc;
                    post.minv_column(c, [&](int t, int cc, double v) {
                        const double sg = s2 * v;
                        if (cov) {
                            cov[t * K + cc] = sg;
                            cov[cc * K + t] = sg;
                        }
                        if (rec) rec[K + 1 + tri(t, cc)] = w * fma(z[t], zc, sg);
                    });
                }
            }
        }
    }

    // the scalars: butterflies over the wave (the same total on every lane), then the waves in order
    sw = wave_sum(sw);
    swl = wave_sum(swl);
    sne = wave_sum(sne);
    sbad = wave_sum(sbad);
    if (lane == 0) {
        sred[wave][0] = sw;
        sred[wave][1] = swl;
        sred[wave][2] = sne;
        sred[wave][3] = sbad;
    }
    __syncthreads();
    if (tid < 4) a.scal[(int64_t)blockIdx.x * 4 + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

struct HStatsArgs {
    const double *X, *P;
    int64_t ldx, ldp, n;
    int d;
    const double *model;
    const double *rec;  // n x NRP
    double *part;       // [nsplit][hetero_stats_len]
    int tiles;
    int64_t rows_per;   // a multiple of H_SR
};

template <int K>
__global__ __launch_bounds__(H_THREADS) void hetero_stats_kernel(HStatsArgs a) {
    using Cf = HCfg<K>;
    constexpr int NS = H_SR / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int d = a.d;
    // the column tiles of one row run read the same records: on the same XCD (workgroups go round the eight XCDs), one after the other
    const unsigned nb = gridDim.x, job = nb % 8u == 0u ? (blockIdx.x % 8u) * (nb / 8u) + blockIdx.x / 8u : blockIdx.x;
    const int tile = (int)(job % (unsigned)a.tiles), split = (int)(job / (unsigned)a.tiles);
    const int j = tile * H_CT + 16 * wave + l15;
    const bool jok = j < d;
    const int jc = jok ? j : d - 1;
    const double muj = a.model[MODEL_HDR + (int64_t)d * K + jc];
    const int64_t r0 = (int64_t)split * a.rows_per, r1 = r0 + a.rows_per < a.n ? r0 + a.rows_per : a.n;
    const double qnan = __builtin_nan("");

    d4h_t accS[Cf::NRB], accX[Cf::NCB];
#pragma unroll
    for (int t = 0; t < Cf::NRB; ++t) accS[t] = d4h_t{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < Cf::NCB; ++t) accX[t] = d4h_t{0, 0, 0, 0};
    double sq = 0.0, cnt = 0.0;

    for (int64_t rb = r0; rb < r1; rb += H_SR) {
        double x[NS], p[NS], wv[NS], b[NS][Cf::NRB];
#pragma unroll
        for (int s = 0; s < NS; ++s) {  // every load of the step before the first product
            const int64_t i = rb + 4 * s + l4;
            const bool rok = i < r1;
            const int64_t ic = rok ? i : r1 - 1;
            x[s] = rok && jok ? __builtin_nontemporal_load(a.X + ic * a.ldx + jc) : qnan;
            p[s] = rok && jok ? __builtin_nontemporal_load(a.P + ic * a.ldp + jc) : 0.0;
            const double *rr = a.rec + ic * Cf::NRP;
#pragma unroll
            for (int t = 0; t < Cf::NRB; ++t) {
                const double v = rr[16 * t + l15];
                b[s][t] = rok ? v : 0.0;
            }
            const double w = rr[K];
            wv[s] = rok ? w : 0.0;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool o = h_observed(x[s], p[s]);
            const double xt = o ? __dsub_rn(x[s], muj) : 0.0;
            const double pv = o ? p[s] : 0.0;
            const double px = __dmul_rn(pv, xt);
#pragma unroll
            for (int t = 0; t < Cf::NRB; ++t) {
                accS[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(pv, b[s][t], accS[t], 0, 0, 0);
                if (t < Cf::NCB) accX[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(px, b[s][t], accX[t], 0, 0, 0);
            }
            sq = fma(__dmul_rn(wv[s], px), xt, sq);
            cnt += o ? wv[s] : 0.0;
        }
    }

    // the job's own columns of part[split]: cross (d x k) | S (d x kp) | V (d x k) | A | T | sq | cnt
    const int64_t oS = (int64_t)d * K, oV = oS + (int64_t)d * Cf::KP, oA = oV + (int64_t)d * K, oT = oA + d, oQ = oT + d, oC = oQ + d;
    double *part = a.part + (int64_t)split * (oC + d);
#pragma unroll
    for (int t = 0; t < Cf::NRB; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int jo = tile * H_CT + 16 * wave + l4 + 4 * q, e = 16 * t + l15;
            if (jo >= d) continue;
            if (e < K) {
                part[oV + (int64_t)jo * K + e] = accS[t][q];
                if (t < Cf::NCB) part[(int64_t)jo * K + e] = accX[t][q];
            } else if (e == K) {
                part[oT + jo] = accS[t][q];
                if (t < Cf::NCB) part[oA + jo] = accX[t][q];
            } else if (e < Cf::NR) {
                part[oS + (int64_t)jo * Cf::KP + (e - K - 1)] = accS[t][q];
            }
        }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    cnt += __shfl_xor(cnt, 16, 64);
    cnt += __shfl_xor(cnt, 32, 64);
    if (l4 == 0 && jok) {
        part[oQ + j] = sq;
        part[oC + j] = cnt;
    }
}

// out = mean + C z (mode 0), or x where the entry is observed (mode 1)
__global__ __launch_bounds__(256) void hetero_recon_kernel(const double *X, int64_t ldx, const double *P, int64_t ldp, int64_t n, int d, int k,
                                                           const double *model, const double *states, int mode, double *out) {
    const double *C = model + MODEL_HDR, *mu = C + (int64_t)d * k;
    const int64_t total = n * d, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int64_t r = idx / d;
        const int j = (int)(idx - r * d);
        double dot = 0.0;
        for (int b = 0; b < k; ++b) dot = fma(C[(int64_t)j * k + b], states[r * k + b], dot);
        double v = mu[j] + dot;
        if (mode == 1) {
            const double x = __builtin_nontemporal_load(X + r * ldx + j), p = __builtin_nontemporal_load(P + r * ldp + j);
            v = h_observed(x, p) ? x : v;
        }
        __builtin_nontemporal_store(v, out + idx);
    }
}

template <int K>
hipError_t sweep_t(const HSweepArgs &a, int grid, hipStream_t s) {
    const size_t lds = sizeof(double) * HCfg<K>::LDS_DOUBLES;
    if (hipError_t e = ensure_dynamic_lds<hetero_sweep_kernel<K>>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((hetero_sweep_kernel<K>), dim3((unsigned)grid), dim3(H_THREADS), lds, s, a);
    return hipGetLastError();
}
template <int K>
hipError_t stats_t(const HStatsArgs &a, int grid, hipStream_t s) {
    hipLaunchKernelGGL((hetero_stats_kernel<K>), dim3((unsigned)grid), dim3(H_THREADS), 0, s, a);
    return hipGetLastError();
}

#define H_DISPATCH(k, F, ...)                   \
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

}  // namespace

bool hetero_covers(int d, int k) { return d >= 1 && d <= HETERO_MAX_D && k >= 1 && k <= HETERO_MAX_K; }
int hetero_ntp(int k) { return h_ntp(k); }
int hetero_nrp(int k) { return h_nrp(k); }
int64_t hetero_stats_len(int d, int k) { return (int64_t)d * (2 * k + k * (k + 1) / 2 + 4); }

int hetero_sweep_grid(int64_t n, int n_cu) {
    if (n <= 0) return 0;
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(n_cu, 1) * 2, (n + H_ROWS - 1) / H_ROWS));
}

HeteroPlan hetero_stats_plan(int64_t n, int d, int n_cu) {
    HeteroPlan p{};
    p.tiles = (d + H_CT - 1) / H_CT;
    const int64_t want = std::max<int64_t>(1, ((int64_t)std::max(n_cu, 1) * 6 + p.tiles - 1) / p.tiles);  // ~6 jobs per CU: 2 or 3 rounds of the resident workgroups
    p.nsplit_max = (int)want;
    if (n <= 0) return p;
    const int64_t per = (n + want - 1) / want;
    p.rows_per = (per + H_SR - 1) / H_SR * H_SR;
    p.nsplit = (int)((n + p.rows_per - 1) / p.rows_per);
    return p;
}

hipError_t launch_hetero_table(const double *model, int d, int k, double *tab, hipStream_t s) {
    if (!hetero_covers(d, k)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)d * h_ntp(k);
    hipLaunchKernelGGL(hetero_table_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, model, d, k, tab);
    return hipGetLastError();
}

hipError_t launch_hetero_sweep(const double *X, int64_t ldx, const double *P, int64_t ldp, const double *w, int64_t n, int d, int k,
                               const double *model, const double *tab, double *llks, double *states, double *covs, double *rec,
                               double *scal_part, int grid, hipStream_t s) {
    if (n <= 0 || grid <= 0) return hipSuccess;
    if (!hetero_covers(d, k)) return hipErrorInvalidValue;
    const int64_t per = ((n + grid - 1) / grid + H_ROWS - 1) / H_ROWS * H_ROWS;
    const HSweepArgs a{X, P, ldx, ldp, n, d, w, model, tab, llks, states, covs, rec, scal_part, per};
    H_DISPATCH(k, sweep_t, a, grid, s);
}

hipError_t launch_hetero_stats(const double *X, int64_t ldx, const double *P, int64_t ldp, int64_t n, int d, int k, const double *model,
                               const double *rec, const HeteroPlan &p, double *part, hipStream_t s) {
    if (n <= 0 || p.nsplit <= 0) return hipSuccess;
    if (!hetero_covers(d, k)) return hipErrorInvalidValue;
    const HStatsArgs a{X, P, ldx, ldp, n, d, model, rec, part, p.tiles, p.rows_per};
    const int grid = p.nsplit * p.tiles;
    H_DISPATCH(k, stats_t, a, grid, s);
}

hipError_t launch_hetero_recon(const double *X, int64_t ldx, const double *P, int64_t ldp, int64_t n, int d, int k, const double *model,
                               const double *states, int mode, double *out, int n_cu, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n * d + 255) / 256, (int64_t)std::max(n_cu, 1) * 16);
    hipLaunchKernelGGL(hetero_recon_kernel, dim3((unsigned)blocks), dim3(256), 0, s, X, ldx, P, ldp, n, d, k, model, states, mode, out);
    return hipGetLastError();
}

}  // namespace ppca
