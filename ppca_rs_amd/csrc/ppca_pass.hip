// ppca_pass.hip -- the four-wave fused pass of the PPCA EM hot path on gfx950 (CDNA4) and its launchers.
//
// pass_kernel<K, EM, GI8>: ONE streaming pass over the sample matrix X that fuses what
// the reference does in five sweeps (reference = viodotcom/ppca_rs):
//   infer            ppca/src/ppca_model.rs:221-227 (infer_one :195-208)
//   cross moment     :281-293
//   second moments   :294-306   (the reference's d sequential scans over N)
//   noise 4-tuple    :328-358
//   llk              :142-149
// Persistent workgroups (one per CU) walk tiles of 32 samples:
//   P1  coalesced row loads (prefetched one tile ahead in registers) ->
//       x~ = observed ? x - mean : 0 into an LDS tile, mask words by wave ballot
//   P2  [G | b] = [Mask | X~] (32 x 256) . [vech(c c^T) | C] (256 x (k'+k))
//       on v_mfma_f64_16x16x4_f64 (true dense contractions over the 256 dims)
//   P3  per-sample k x k SPD solve, one lane per sample, registers only:
//       z, Sigma, ln det, quadratic form -> llk, noise terms, w P, w z
//   P4  S/U/totals (256 x (k'+k+1)) += Mask^T . [wP | wz | w],
//       cross/sumx (256 x (k+1))   += X~^T  . [wz | w]   on fp64 MFMA,
//       accumulators persistent in registers across all tiles of the workgroup
// and end with one deterministic per-workgroup partial that reduce_partials sums
// in fixed order.  No atomics: results are bit-reproducible for a given grid.
// The kernels before and after a pass -- the slice table and its guard (launch_qprep), the reductions, the finalisation -- are
// ppca_kernels.hip's, reached through their launchers (ppca_internal.hpp).
#include <type_traits>
#include <utility>

#include "ppca_sweep.hpp"

namespace ppca {

// Four waves per workgroup (one per SIMD, 512 registers each).  Instantiated as <K, false, true> (the int8-Gram output pass),
// <K, false, false> and <K, true, false> (the fp64-Gram output and EM passes: the pinned fp64 engine and the fallback behind
// the guards); the int8-Gram EM pass is em9_kernel.
// GI8: Gram on the int8 MFMA (wave t <-> packed-column tile t) instead of fp64 MFMA; output passes only.
// The EM pass honours PassArgs::rows (sample i = physical row rows[i]).
template <int K, bool EM, bool GI8>
__global__ __launch_bounds__(256) void pass_kernel(PassArgs p) {
    using cfg = Cfg<K>;
    constexpr int KP = cfg::KP, NTP = cfg::NTP, NTM = cfg::NTM, B = cfg::B, XS = cfg::XS, CS = cfg::CS,
                  GS = cfg::GS, WS = cfg::WS;
    constexpr int THREADS = 256;         // four waves: one per SIMD, 512 registers each
    constexpr int RPW = B / 4;           // rows staged per wave in P1
    constexpr int DPS = cfg::DP / 2;     // dims per K-split of the [G | b] contraction (2 splits x 2 row tiles = 4 waves)
    constexpr int STEPS = DPS / 4;       // MFMA k-steps per split
    constexpr int RT = 4;                // accumulator row tiles (16 dims each) per wave in P4
    constexpr int DW = cfg::DP / 4;      // dims owned by a wave in P4
    // Mask-side columns of P4: k' (vech P) + k (w z) + 1 (w).  When they overflow the k' tiles by at most four
    // columns (k = 10: 66 = 4 x 16 + 2) the first PADS of [w z | w] ride in the padding of the last vech tile and
    // the remaining SMALL_COLS go through v_mfma_f64_4x4x4_4b (four 4 x 4 x 4 blocks, 18 cycles) instead of a
    // fifth 16-column tile of 64-cycle MFMAs: 16 + 4 instead of 20 big MFMAs per k-step and wave.
    constexpr int PADS = 16 * NTP - KP;
    constexpr int SMALL_COLS = K + 1 - PADS;
    constexpr bool SPLIT = EM && SMALL_COLS > 0 && SMALL_COLS <= 4 && PADS > 0;
    constexpr int NTMB = SPLIT ? NTP : NTM;  // big (16-column) mask-side tiles
    static_assert(!GI8 || (!EM && NTP <= 4), "int8 Gram: output pass only, one wave per packed-column tile");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double *Xs = sm + cfg::OFF_X;
    double *Cs = sm + cfg::OFF_C;
    double *Gp = sm + cfg::OFF_G;
    double *Ws = sm + cfg::OFF_W;
    unsigned long long *Ms = reinterpret_cast<unsigned long long *>(sm + cfg::OFF_M);
    double *xxs = sm + cfg::OFF_S;

    const int *prows = p.rows;
    const double *pw = p.w;
    const int *pndev = p.n_dev;
    const int64_t pn = p.n;
    int fb_mode = 0;  // second stage of a guarded EM pass: reduce_wguard_kernel's verdict (Gram flags or the W-side check)
    if (!GI8 && p.runflag) {
        fb_mode = *p.runflag;
        if (fb_mode == 0) return;
    } else if (p.qflag) {  // Gram engine chosen per model by qprep's dynamic-range guard: exactly one of the two variants runs
        int unsafe = 0;
#pragma unroll
        for (int t = 0; t < NTP; ++t) unsafe |= p.qflag[t];
        if (GI8 == (unsafe != 0)) return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: row bases stay in SGPRs
    const int l15 = lane & 15, l4 = lane >> 4;
    const int d = p.d;
    const int64_t n = pndev ? (int64_t)*pndev : pn;
    const double *mC = p.model + MODEL_HDR;
    const double *mMean = mC + (int64_t)d * K;
    const double s2 = p.model[1], lnsig = p.model[2];

    for (int idx = tid; idx < cfg::DP * CS; idx += THREADS) {
        int j = idx / CS, a = idx - j * CS;
        Cs[idx] = (j < d && a < K) ? mC[(int64_t)j * K + a] : 0.0;
    }
    for (int idx = tid; idx < B * WS; idx += THREADS) Ws[idx] = 0.0;

    double muo[4];  // means in the output pass's lane map (dim = 64 wave + 16 c4 + lane % 16)
    if constexpr (!EM) {
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const int j = 64 * (wave & 3) + 16 * c4 + l15;
            muo[c4] = (j < d) ? mMean[j] : 0.0;
        }
    }
    // Staging lane map: a row arrives as two 16-byte loads per lane, lane l holding dims 128 h + 2 l + e
    // (element q = 2 h + e): half as many memory and LDS-store instructions as 8-byte loads of dims 64 q + l.
    double mu[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int j = 128 * (q >> 1) + 2 * lane + (q & 1);
        mu[q] = (j < d) ? mMean[j] : 0.0;
    }
    // (a, b) of packed column c = 16 t + (lane & 15); pad columns point at the zero column K
    int pa[NTP], pb[NTP];
#pragma unroll
    for (int t = 0; t < NTP; ++t) {
        int c = 16 * t + l15;
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= c) ++a;
        int b = c - a * (a + 1) / 2;
        if (c >= KP) { a = K; b = K; }
        pa[t] = a;
        pb[t] = b;
    }
    const int colb = (l15 < K) ? l15 : K;

    d4_t accM[RT][NTM];
    double accS[RT];  // SPLIT: the 4-column group, D lane = 16 i + 4 block + j (dim 4 block + i of the row tile, column j)
    d4_t accX[RT];
    if constexpr (EM) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
#pragma unroll
            for (int t = 0; t < NTM; ++t) accM[r][t] = d4_t{0, 0, 0, 0};
            accS[r] = 0.0;
            accX[r] = d4_t{0, 0, 0, 0};
        }
    }
    // unweighted EM pass: sum_i ln det M_i = ln prod_i det M_i, so each solver lane keeps a running
    // (mantissa, exponent) product and takes ONE logarithm at the end of the kernel (a per-tile fp64 log
    // cost 2.2k of ~35k cycles per tile: its constants live in scratch at this register pressure)
    double *scl = sm + cfg::OFF_L;
    // PAIRS: the M^-1 columns are computed two at a time, by lane i (column 2p) and lane i + 32 (column 2p + 1)
    constexpr bool PAIRS = EM && K >= 2;
    constexpr int SQW = PAIRS ? 2 * B : B;  // sq slots per wave
    constexpr int L_DEV = 4 * SQW, L_LLK = L_DEV + B, L_W = L_DEV + 2 * B, L_NE = L_DEV + 3 * B, L_PM = L_DEV + 4 * B,
                  L_PX = L_DEV + 5 * B;
    for (int idx = tid; idx < L_DEV + 6 * B; idx += THREADS) scl[idx] = (idx >= L_PM && idx < L_PX) ? 1.0 : 0.0;
    const double inv_s2 = 1.0 / s2;

    const int64_t ntiles = (n + B - 1) / B;
    double xr[RPW][4];
    // Row loads are unconditional (clamped to real rows; nothing between issue and first use, so a whole
    // tile's loads stay in flight); out-of-range rows / dims are masked when consumed in P1.
    // observed <=> |x| < lim: +inf for a real dimension (finite test, dataset.rs:19-22), -1 for the padding past d
    double lim[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) lim[q] = (128 * (q >> 1) + 2 * lane + (q & 1) < d) ? __builtin_inf() : -1.0;
    // Each workgroup walks a CONTIGUOUS run of tiles (consecutive 64 KB pieces of X share pages, unlike a
    // grid-strided walk that starts every tile 16 MB further on).
    const int64_t tiles_per_wg = (ntiles + gridDim.x - 1) / gridDim.x;
    int64_t tile_begin = (int64_t)blockIdx.x * tiles_per_wg;
    int64_t tile_end = tile_begin + tiles_per_wg < ntiles ? tile_begin + tiles_per_wg : ntiles;
    if (!GI8 && fb_mode == 2) {
        // Only the slices of the flagged workgroups of the guarded launch (same grid: slice g = tiles [g tpw, (g + 1) tpw)), each
        // split over gridDim.x / n_flagged workgroups of this one: a workgroup's run stays inside ONE slice, so everything below
        // (descriptors relative to the run's first row, weights, gather list) is the plain pass's.
        const int nfl = p.runflag[QF_NFLAGGED - QF_MODE];
        const int wps = (int)gridDim.x / nfl, f = (int)blockIdx.x / wps, sub = (int)blockIdx.x - f * wps;
        if (f >= nfl) {
            tile_begin = tile_end = 0;
        } else {
            const int64_t s0 = (int64_t)p.who[f] * tiles_per_wg, s1 = s0 + tiles_per_wg < ntiles ? s0 + tiles_per_wg : ntiles;
            const int64_t per = (s1 - s0 + wps - 1) / wps;
            tile_begin = s0 + (int64_t)sub * per;
            tile_end = tile_begin + per < s1 ? tile_begin + per : s1;
            if (tile_begin > tile_end) tile_begin = tile_end;
        }
    }
    const int64_t nleft = n - tile_begin * B;
    const int nrel = (int)(nleft < (1 << 30) ? nleft : (1 << 30));  // rows from the workgroup's first row to the end
    const double *Xwg = p.X + tile_begin * B * p.ldx;
    // real rows of the workgroup's own tiles, counted from its first row
    const int64_t own = (tile_end - tile_begin) * B;
    const int nmine = tile_end > tile_begin ? (int)(own < nleft ? own : nleft) : 0;
    constexpr bool ROW_LIST = EM;  // the EM pass honours PassArgs::rows
    const int *rows_wg = (ROW_LIST && prows) ? prows + tile_begin * B : nullptr;
    const int lane_entry = lane;
    // Row loads are buffer loads through ONE descriptor per tile (base = the tile's first row, extent = its real rows;
    // rows are contiguous, ldx == d): the row is a scalar offset, the lane offset one constant VGPR, the half an
    // immediate -- no vector address arithmetic and no per-row scalar work.  Rows past n read as zeros: "observed",
    // but weighted with zero or skipped by every consumer.  The gathered pass (PassArgs::rows: sample i = physical
    // row rows[i]) builds a descriptor per row from one scalar load.
    const int rowbytes = d * (int)sizeof(double);
    auto tile_rsrc = [&](int64_t tile) {
        const int rel0 = (int)(tile - tile_begin) * B;
        int cnt = nrel - rel0;
        cnt = __builtin_amdgcn_readfirstlane(cnt < 0 ? 0 : (cnt > B ? B : cnt));  // (keeps the descriptor scalar)
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(Xwg + (int64_t)rel0 * p.ldx), 0, cnt * rowbytes, 0x00020000);
    };
    auto load_row = [&](const __amdgpu_buffer_rsrc_t &trs, int64_t tile, int r) {
        typedef unsigned u4_t __attribute__((ext_vector_type(4)));
        if constexpr (ROW_LIST) {
            if (rows_wg) {
                const int rel = (int)(tile - tile_begin) * B + wave * RPW + r;
                const int rc = rel < nrel ? rel : nrel - 1;
                const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<double *>(p.X + (int64_t)rows_wg[rc] * p.ldx), 0, rowbytes, 0x00020000);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u4_t v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, lane_entry * 16, 1024 * h, 0);
                    xr[r][2 * h] = __longlong_as_double(((long long)v[1] << 32) | v[0]);
                    xr[r][2 * h + 1] = __longlong_as_double(((long long)v[3] << 32) | v[2]);
                }
                return;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // validity is applied by the consumers (P1: lim; P3 / outputs: row < n)
            const u4_t v = __builtin_amdgcn_raw_buffer_load_b128(trs, lane_entry * 16, (wave * RPW + r) * rowbytes + 1024 * h, 0);
            xr[r][2 * h] = __longlong_as_double(((long long)v[1] << 32) | v[0]);
            xr[r][2 * h + 1] = __longlong_as_double(((long long)v[3] << 32) | v[2]);
        }
    };
    auto load_tile = [&](int64_t tile) {
        const __amdgpu_buffer_rsrc_t trs = tile_rsrc(tile);
#pragma unroll
        for (int r = 0; r < RPW; ++r) load_row(trs, tile, r);
    };
    if (tile_begin < tile_end) load_tile(tile_begin);
    // int8 Gram: the slice table of this wave's column tile (QS x 4 fragments of 16 B per lane, L2-resident) is read
    // in four digit pairs.  Buffer loads: one scalar resource for the table, a scalar offset per fragment
    // and one lane offset register.  (The wave's table base is made opaque per use: 32 loop-invariant
    // scalar offsets would be hoisted, overflow the SGPR file and come back through v_readlane + s_nop 4.)
    static_assert(!GI8 || QS == 8, "digit grouping below assumes 8 slices");
    const __amdgpu_buffer_rsrc_t qrsrc = __builtin_amdgcn_make_buffer_rsrc(p.qtab, 0, (int)qtab_bytes<K>(), 0x00020000);
    // Waves without a column tile (k' <= 48) run the same loads (out of range of the table: zeros) and MFMAs
    // and skip only the final store: a run-time condition around the loads would make the fragment registers
    // look live around the whole tile loop.
    const bool gram_wave = GI8 && (NTP >= 4 || wave < NTP);  // compile-time true when every wave owns a tile
    auto load_pair = [&](i4_t(&dst)[2][4], int sl0) {
        int qbase = wave * QS * 4 * 1024;
        asm volatile("" : "+s"(qbase));
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                typedef unsigned u4_t __attribute__((ext_vector_type(4)));
                // (the k-chunk rides in the instruction's immediate offset: one scalar offset per slice, not per fragment)
                const u4_t v = __builtin_amdgcn_raw_buffer_load_b128(qrsrc, lane_entry * 16 + kc * 1024, qbase + (sl0 + u) * 4096, 0);
                dst[u][kc] = i4_t{(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
            }
    };
    // The int8 Gram serves output passes only: no statistics accumulators, so the wave's whole slice of the table
    // (QS x 4 fragments = 128 registers) is loaded once per workgroup and stays resident -- no table traffic inside
    // the tile loop.
    i4_t qt[GI8 ? QS : 1][4];
    if constexpr (GI8) {
#pragma unroll
        for (int sl = 0; sl < QS; sl += 2) load_pair(*reinterpret_cast<i4_t(*)[2][4]>(&qt[sl]), sl);
    }
#ifdef PPCA_PHASE_TIMING
    long long tph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast = clock64();
#define PPCA_STAMP(i) { long long tn = clock64(); tph[i] += tn - tlast; tlast = tn; }
#elif defined(PPCA_MARKS)  // tools/devbuild.py -DPPCA_MARKS --asm: phase boundaries as comments in the ISA listing
#define PPCA_STAMP(i) asm volatile("; PPCA_MARK " #i ::: "memory");
#else
#define PPCA_STAMP(i)
#endif
    // ---- P1 as three pieces, so that the EM pass can run it for tile t+1 inside tile t's P4.
    // Wave-uniform results (mask words, popcounts, row sums) are gathered into the lane that will store
    // them -- lane 4r+q keeps mask word q of row r, lane r keeps xx_r / m_r (v_writelane drops each scalar
    // into its lane: 32 "lane == c" compare masks would overflow the SGPR file) -- so the whole wave does
    // ONE compact store per array.
    int st_wlo = 0, st_whi = 0;
    auto stage_begin = [&]() { st_wlo = st_whi = 0; };
    // One row = 7 small pieces that P4 spreads over a k-step: per half h of the row, two "classify + centre" pieces
    // (elements 2h, 2h+1) and one "file" piece (mask words, x~ pair, squares); 6 = the row's |x~|^2.
    // (the EM pass needs only the weighted SUM of the |x~_i|^2 -- sigma^2 and the total llk are linear in it --
    //  so it keeps one running per-lane sum, reduced once per kernel; the output passes keep the eight per-lane
    //  partials of a wave's rows and sum them together in stage_end)
    constexpr int STAGE_PIECES = 7;
    double xx_run = 0.0;
    double pxx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    static_assert(EM || RPW == 8, "output passes: eight staged rows per wave (store_row_sums)");
    double pc_xt0 = 0.0, pc_xt1 = 0.0, pc_xx = 0.0;
    unsigned long long pc_b0 = 0ull, pc_b1 = 0ull;
    auto stage_piece = [&](int64_t t, int lane, auto r_tag, auto p_tag) {
        constexpr int r = decltype(r_tag)::value, P = decltype(p_tag)::value;
        const int ri = wave * RPW + r;
        if constexpr (P == 0 || P == 1 || P == 3 || P == 4) {  // classify + centre element q = 2 h + e
            constexpr int q = (P < 2) ? P : P - 1, e = q & 1;
            if constexpr (q == 0) {
                pc_xx = 0.0;
            }
            // Rows past n (the clamped last row again) and the tile staged behind the workgroup's last P4 (another
            // workgroup's, or none) are staged like any other: every consumer weighs them with zero or skips them.
            // The compare's wave mask IS the ballot and feeds the select directly -- no scalar instruction between.
            const double v = xr[r][q];
            const bool ob = __builtin_fabs(v) < lim[q];
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(ob);
            const double xt = ob ? v - mu[q] : 0.0;  // select, never multiply (utils.rs:118-127)
            if constexpr (e == 0) {
                pc_b0 = bal;
                pc_xt0 = xt;
            } else {
                pc_b1 = bal;
                pc_xt1 = xt;
            }
        } else if constexpr (P == 2 || P == 5) {  // file half h: mask words, x~ pair, sums
            constexpr int h = (P == 2) ? 0 : 1;
            // mask word 2 h + e of the row = the ballot of element 2 h + e (bit l <-> dim 128 h + 2 l + e); the
            // readers index it that way (P2: any order of a sum, qprep lays the table out to match; P4b / output
            // pass: word by the parity of the dimension)
            writelane_mask<4 * r + 2 * h>(st_wlo, st_whi, pc_b0);
            writelane_mask<4 * r + 2 * h + 1>(st_wlo, st_whi, pc_b1);
            typedef double d2_t __attribute__((ext_vector_type(2)));
            *reinterpret_cast<d2_t *>(Xs + ri * XS + 128 * h + 2 * lane) = d2_t{pc_xt0, pc_xt1};  // 16-byte aligned
            pc_xx += pc_xt0 * pc_xt0;
            pc_xx += pc_xt1 * pc_xt1;
        } else if constexpr (P == 6) {
            if constexpr (!EM) pxx[r] = pc_xx;  // the per-sample |x~|^2: the eight rows are summed together in stage_end
            if constexpr (EM) {
                // wave-uniform: a real row of one of THIS workgroup's tiles (32-bit compare on the scalar unit)
                const bool mine = (int)(t - tile_begin) * B + ri < nmine;
                const double wr = mine ? (pw ? pw[t * B + ri] : 1.0) : 0.0;  // (scalar load)
                xx_run += wr * pc_xx;
            }
        }
    };
    auto stage_row = [&](int64_t t, int lane, auto r_tag) {
        static_for<STAGE_PIECES>([&](auto p_tag) { stage_piece(t, lane, r_tag, p_tag); });
    };
    auto stage_end = [&](int lane, int par) {
        const unsigned long long myw = ((unsigned long long)(unsigned)st_whi << 32) | (unsigned)st_wlo;
        if (lane < 4 * RPW) Ms[par * 4 * B + wave * 4 * RPW + lane] = myw;
        if constexpr (!EM) store_row_sums(pxx, lane, xxs + wave * RPW);
    };
    if constexpr (EM) {
        if (tile_begin < tile_end) {
            stage_begin();
            static_for<RPW>([&](auto r_tag) { stage_row(tile_begin, lane, r_tag); });
            stage_end(lane, 0);
        }
        __syncthreads();
    }
    for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
        // The lane index is made opaque once per tile: everything derived from it (LDS addresses, shift
        // counts, column maps) is then recomputed per tile -- a few integer ops -- instead of being
        // hoisted out of the loop by LICM and parked in (spilled) registers for the whole kernel.
        int lane = lane_entry;
        asm volatile("" : "+v"(lane));
        const int l15 = lane & 15, l4 = lane >> 4;
        const int colb = (l15 < K) ? l15 : K;
        // ------------------------------------------------------------ P1
        // EM: the tile was staged behind the previous tile's P4 (or before the loop for the first one)
        if constexpr (!EM) {
            stage_begin();
            static_for<RPW>([&](auto r_tag) { stage_row(tile, lane, r_tag); });
            PPCA_STAMP(5)
            stage_end(lane, 0);
            __syncthreads();
        }
        const unsigned long long *Msc = Ms + (EM ? (int)((tile - tile_begin) & 1) * 4 * B : 0);
        PPCA_STAMP(0)
        // ------------------------------------------------------------ P2
        {
            const int rt = wave & 1, kq = wave >> 1;
            const int si = 16 * rt + l15;
            // fp64 Gram: the lane's dims DPS kq + 4 s + l4 all sit in ONE mask word (parity l4 & 1), bits 2 s apart
            const unsigned long long mwsel = Msc[si * 4 + 2 * ((DPS * kq) >> 7) + (l4 & 1)];
            const int mwbit = (((DPS * kq) & 127) >> 1) + (l4 >> 1);
            d4_t acc[NTM];
#pragma unroll
            for (int t = 0; t < NTM; ++t) acc[t] = d4_t{0, 0, 0, 0};
            // lane-constant base pointers; after full unrolling every LDS read below is
            // base + immediate offset (no per-step address arithmetic)
            const double *xrow = Xs + si * XS + DPS * kq + l4;
            const double *crow = Cs + (DPS * kq + l4) * CS;
            const double *cpa[NTP], *cpb[NTP];
#pragma unroll
            for (int t = 0; t < NTP; ++t) {
                cpa[t] = crow + pa[t];
                cpb[t] = crow + pb[t];
            }
            const double *cpc = crow + colb;
            // A = mask bytes: lane (sample = 16 rt + l15, dims 64 kc + 16 l4 .. +15); 4 bits -> 4 bytes
            // by one multiply: (x * 0x204081) & 0x01010101 puts bit i of x into byte i.
            i4_t af[2][4];
            double v[2][4];
            // one digit pair: contract, then fold the (exact) integer digit sums -- |sum| <= 2^14, so two
            // digits fit one i32 with room to spare -- into the running fp64 value, Horner in 128^2
            auto group = [&](const i4_t(*qb)[4], bool first) {
#pragma unroll
                for (int rt2 = 0; rt2 < 2; ++rt2) {
                    i4_t ia[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        ia[u] = i4_t{0, 0, 0, 0};
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc)
                            ia[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[rt2][kc], qb[u][kc], ia[u], 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int part = ia[1][r] * QBASE + ia[0][r];
                        v[rt2][r] = first ? (double)part : v[rt2][r] * (double)(QBASE * QBASE) + (double)part;
                    }
                }
            };
            double qs = 0.0;
            if constexpr (GI8) {
                {
                    // (the mask words are requested from LDS first, so that their latency runs under the issue of
                    //  the table loads)
                    unsigned long long mwd[2][4];
#pragma unroll
                    for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc) mwd[rt2][kc] = Msc[(16 * rt2 + l15) * 4 + kc];
                    __builtin_amdgcn_sched_barrier(0);
                    if (gram_wave) qs = p.qscale[16 * wave + l15];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc) {
                            const unsigned bits = (unsigned)(mwd[rt2][kc] >> (16 * l4)) & 0xFFFFu;
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                af[rt2][kc][u] = (int)((((bits >> (4 * u)) & 0xFu) * 0x00204081u) & 0x01010101u);
                        }
                    PPCA_STAMP(12)
                    group(qt + 6, true);   // digits {7,6}
                    group(qt + 4, false);  // digits {5,4}
                }
            }
            PPCA_STAMP(13)
            if constexpr (GI8) {
                // b = X~ C alone: operands of the next four k-steps are requested before the current four
                // MFMAs issue (hipcc otherwise reads each pair right before its MFMAs and waits on LDS)
                constexpr int CH = 4;
                double axb[2][CH], cbb[2][CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    axb[0][u] = xrow[4 * u];
                    cbb[0][u] = cpc[4 * u * CS];
                }
#pragma unroll
                for (int c = 0; c < STEPS / CH; ++c) {
                    if (c + 1 < STEPS / CH) {
#pragma unroll
                        for (int u = 0; u < CH; ++u) {
                            axb[(c + 1) & 1][u] = xrow[4 * ((c + 1) * CH + u)];
                            cbb[(c + 1) & 1][u] = cpc[4 * ((c + 1) * CH + u) * CS];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);  // (without the fences the reads sink back to their uses)
#pragma unroll
                    for (int u = 0; u < CH; ++u) acc[NTP] = mfma(axb[c & 1][u], cbb[c & 1][u], acc[NTP]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int s = 0; s < (GI8 ? 0 : STEPS); ++s) {
                const double ax = xrow[4 * s];
                if constexpr (!GI8) {
                    const double am = ((mwsel >> (mwbit + 2 * s)) & 1ull) ? 1.0 : 0.0;
#pragma unroll
                    for (int t = 0; t < NTP; ++t)
                        acc[t] = mfma(am, cpa[t][4 * s * CS] * cpb[t][4 * s * CS], acc[t]);
                }
                acc[NTP] = mfma(ax, cpc[4 * s * CS], acc[NTP]);
            }
            PPCA_STAMP(14)
            if constexpr (GI8) {
                group(qt + 2, false);  // digits {3,2}
                group(qt + 0, false);  // digits {1,0}
                if (gram_wave) {
#pragma unroll
                    for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
                        for (int r = 0; r < 4; ++r)  // C/D map of the 16x16 integer MFMA: row = 4 (lane >> 4) + reg
                            Gp[(16 * rt2 + 4 * l4 + r) * GS + 16 * wave + l15] = v[rt2][r] * qs;
                }
            }
            // K-split partials -> two buffers, summed by their readers in a fixed order (deterministic): G = p0 + p1
            // (kq is 0 or 1, which the compiler cannot see behind the readfirstlane of `wave`: the mask and the test are
            //  instructions of the kernels as measured, so they stay)
            double *g = Gp + (kq & 1) * B * GS;
            constexpr int T0 = GI8 ? NTP : 0;  // int8 Gram: only the b tile comes from the fp64 accumulators
            if (kq < 2) {
#pragma unroll
                for (int t = T0; t < NTM; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[(16 * rt + l4 + 4 * r) * GS + 16 * t + l15] = acc[t][r];
            }
        }
        __syncthreads();
        PPCA_STAMP(1)
        if constexpr (!EM) load_tile(tile + 1);  // unconditional: rows are clamped, see load_tile
        // ------------------------------------------------------------ P3
        // Every wave factors every sample (lane = sample, redundantly, in parallel) and the waves
        // share the independent columns of M^-1; wave 0 also owns z, llk and the scalars.
        if (PAIRS || lane < B) {
            const int i = lane & (B - 1);
            const int hi = PAIRS ? lane >> 5 : 0;  // which column of a pair this half of the wave solves for
            const int64_t row = tile * B + i;
            const double *g0 = Gp + i * GS;
            const double *g1 = g0 + B * GS;
            const double wgt = (row < n) ? (pw ? pw[row] : 1.0) : 0.0;
            // observed count of the sample: popcount of its four mask words (the padding past d is never set)
            const int m = __popcll(Msc[i * 4]) + __popcll(Msc[i * 4 + 1]) + __popcll(Msc[i * 4 + 2]) + __popcll(Msc[i * 4 + 3]);
            double *wrow = Ws + i * WS;
            double sc_sq = 0.0, sc_dev = 0.0, sc_llk = 0.0, sc_w = 0.0, sc_ne = 0.0;  // this tile's terms
            const double sq_run = scl[wave * SQW + (PAIRS ? lane : i)];
            Posterior<K> post;
            double pm;
            int pe;
            post.factor([&](int e) { return GI8 ? g0[e] : g0[e] + g1[e]; }, s2, pm, pe);
            PPCA_STAMP(8)
            double z[K], quad, zz;
            post.solve([&](int a) { return g0[16 * NTP + a] + g1[16 * NTP + a]; }, z, quad, zz);
            PPCA_STAMP(9)
            double trpart = 0.0;
            // llk / llks / states / smooth / extrapolate need z only: the posterior covariance (the M^-1 columns)
            // is computed when somebody reads it -- covariances out, or the covariance diagonals
            const bool need_cov = EM || p.covs != nullptr || (p.recon != nullptr && p.recon_mode >= 2);
            if constexpr (PAIRS) {
#pragma unroll
                for (int pp = 0; pp < (K + 1) / 2; ++pp) {
                    if (pair_owner(K, pp, 4) != wave) continue;
                    const int c0 = 2 * pp;
                    const double zc = (hi && c0 + 1 < K) ? z[c0 + 1 < K ? c0 + 1 : c0] : z[c0];
                    // P = z z^T + Sigma, Sigma = sigma^2 M^-1 (ppca_model.rs:437-439), weighted;
                    // tri(t, c0) + 1 = tri(t, c0 + 1)
                    trpart += post.minv_column_pair(c0, hi, [&](int t, double v, bool ok) {
                        if (ok && c0 + hi < K) wrow[tri(t, c0) + hi] = wgt * (z[t] * zc + s2 * v);
                    });
                }
            }
#pragma unroll
            for (int c = 0; c < (PAIRS ? 0 : K); ++c) {
                if (column_owner(K, c, 4) != wave || !need_cov) continue;
                if constexpr (EM) {
                    // P = z z^T + Sigma, Sigma = sigma^2 M^-1 (ppca_model.rs:437-439), weighted
                    trpart += post.minv_column(
                        c, [&](int a, int cc, double v) { wrow[tri(a, cc)] = wgt * (z[a] * z[cc] + s2 * v); });
                } else {
                    trpart += post.minv_column(c, [&](int a, int cc, double v) {
                        const double sv = s2 * v;
                        wrow[K + tri(a, cc)] = sv;  // post mode: W row = [z (K) | Sigma packed (K')]
                    });
                }
            }
            PPCA_STAMP(10)
            if constexpr (EM) {
                // tr(C_o Sigma C_o^T) = <Sigma, G> = s2 (K - s2 tr M^-1)  (:345); each wave carries the
                // share of its columns.  All-masked samples are filtered out of the noise sums (:333).
                if (m > 0) sc_sq -= wgt * s2 * s2 * trpart;
            }
            if (wave == 0 && hi == 0) {
                const double xx = EM ? 0.0 : xxs[i];  // EM: the |x~|^2 terms are added once, in the epilogue
                // running sums: requested at the top of the block, needed at its end
                const double run_dev = scl[L_DEV + i], run_llk = scl[L_LLK + i], run_w = scl[L_W + i], run_ne = scl[L_NE + i];
                const double run_pm = scl[L_PM + i], run_px = scl[L_PX + i];
                if constexpr (EM) {
                    double *zrow = wrow + 16 * NTP;  // W row = [w P (K') | 0.. | w z (K) | w | 0..]
#pragma unroll
                    for (int a = 0; a < K; ++a) zrow[a] = wgt * z[a];
                    zrow[K] = wgt;
                    if constexpr (SPLIT) {  // the leading [w z | w] columns again, in the padding behind vech(P)
#pragma unroll
                        for (int a = 0; a < PADS; ++a) wrow[KP + a] = (a < K) ? wgt * z[a] : wgt;
                    }
                    if (m > 0) {
                        sc_sq += wgt * s2 * (double)K;
                        sc_dev += wgt * (xx - quad - s2 * zz);  // |x~ - C_o z|^2  (:346)
                        sc_ne += (row < n) ? 1.0 : 0.0;
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < K; ++a) wrow[a] = z[a];
                }
                if constexpr (EM) {
                    const double lk0 = sample_llk_nolog(xx, quad, inv_s2, lnsig, m, K);
                    if (pw) {
                        if (!p.no_llk) sc_llk += wgt * (m > 0 ? lk0 - 0.5 * Posterior<K>::logdet(pm, pe) : 0.0);
                    } else {
                        const bool use = m > 0 && row < n;  // wgt is 1 for real rows
                        sc_llk += use ? lk0 : 0.0;
                        int e;
                        scl[L_PM + i] = frexp(run_pm * (use ? pm : 1.0), &e);
                        scl[L_PX + i] = run_px + (double)(e + (use ? pe : 0));
                    }
                    sc_w += wgt;
                } else {
                    const double lk = sample_llk(xx, quad, Posterior<K>::logdet(pm, pe), s2, lnsig, m, K);
                    sc_llk += wgt * lk;
                    sc_w += wgt;
                    if (p.llks && row < n) p.llks[row] = lk;
                }
                scl[L_DEV + i] = run_dev + sc_dev;
                scl[L_LLK + i] = run_llk + sc_llk;
                scl[L_W + i] = run_w + sc_w;
                scl[L_NE + i] = run_ne + sc_ne;
            }
            if constexpr (EM) scl[wave * SQW + (PAIRS ? lane : i)] = sq_run + sc_sq;
        }
        PPCA_STAMP(11)
        __syncthreads();
        PPCA_STAMP(2)
        if constexpr (!EM) {
            // InferredMasked outputs (src/python_bindings.rs:211-234): the tile's states (32 x k) and covariances
            // (32 x k x k) are contiguous in the output arrays, so they are written from the W rows by the whole
            // workgroup with consecutive lanes on consecutive addresses (not 8 bytes per lane 8 k^2 bytes apart)
            if (p.states) {
                for (int idx = tid; idx < B * K; idx += THREADS) {
                    const int i = idx / K, a = idx - i * K;
                    const int64_t row = tile * B + i;
                    if (row < n) p.states[row * K + a] = Ws[i * WS + a];
                }
            }
            if (p.covs) {
                for (int idx = tid; idx < B * K * K; idx += THREADS) {
                    const int i = idx / (K * K), rem = idx - i * (K * K), a = rem / K, c = rem - a * K;
                    const int64_t row = tile * B + i;
                    if (row < n) p.covs[row * (K * K) + rem] = Ws[i * WS + K + (a >= c ? tri(a, c) : tri(c, a))];
                }
            }
        }
        if constexpr (EM) {
            // -------------------------------------------------------- P4
            // (a) cross/sumx += X~^T [wz | w]: the only reader of the x~ tile; the next tile's rows are
            //     requested one per k-step behind these MFMAs (a burst of all of them stalls the wave
            //     ~2.9k cycles on the memory queue: a CU drains ~10 B/cycle)
            PPCA_STAMP(6)
            {
                // operands of step s+1 are read from LDS before the MFMAs of step s issue (fenced: hipcc otherwise
                // sinks the reads to their uses and waits on LDS in front of every step)
                double bzb[2], axb[2][RT];
                const __amdgpu_buffer_rsrc_t trs = tile_rsrc(tile + 1);
                bzb[0] = Ws[l4 * WS + 16 * NTP + l15];
#pragma unroll
                for (int r = 0; r < RT; ++r) axb[0][r] = Xs[l4 * XS + DW * wave + 16 * r + l15];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    if (s < RPW) load_row(trs, tile + 1, s);  // unconditional; two rows per step measured slower
                    if (s + 1 < 8) {
                        const int smp = 4 * (s + 1) + l4;
                        bzb[(s + 1) & 1] = Ws[smp * WS + 16 * NTP + l15];
#pragma unroll
                        for (int r = 0; r < RT; ++r) axb[(s + 1) & 1][r] = Xs[smp * XS + DW * wave + 16 * r + l15];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < RT; ++r) accX[r] = mfma(axb[s & 1][r], bzb[s & 1], accX[r]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();  // the x~ tile is free
            PPCA_STAMP(4)
            // (b) S/U/totals += Mask^T [wP | wz | w], with the staging (P1) of the next tile's rows between the MFMAs
            stage_begin();
            // mask operand of dims DW wave + 16 r + l15: word 2 (dim / 128) + parity, bit (dim % 128) / 2
            const int mword = 2 * ((DW * wave) >> 7) + (l15 & 1);
            unsigned long long mwc = Msc[l4 * 4 + mword];
            double bwc[NTMB], bsc = 0.0;
#pragma unroll
            for (int t = 0; t < NTMB; ++t) bwc[t] = Ws[l4 * WS + 16 * t + l15];
            if constexpr (SPLIT) bsc = Ws[l4 * WS + 16 * NTP + PADS + (lane & 3)];
            // One staging piece follows each MFMA.  Measured (tools/ubench_shadow.hip): v_mfma_f64 holds the
            // SIMD's VALU port for its 64 cycles -- no VALU instruction of this wave overlaps it, only LDS,
            // SALU and memory instructions do -- so this interleave hides the staging's LDS writes and the
            // row-load latency, not its ALU work.  The B operands of step s+1 are read from LDS during step s.
            // B operand of the 4x4x4 blocks: lane = 16 k + 4 block + j -> W[sample 4 s + k][column j of the group];
            // its A operand (lane = 16 k + 4 block + i -> dim 4 block + i, sample k) is the SAME register as the
            // 16x16x4 tiles' (row = lane % 16, k = lane / 16): no extra mask expansion.
            static_for<8>([&](auto s_tag) {
                constexpr int s = decltype(s_tag)::value;
                unsigned long long mwn = 0ull;
                double bwn[NTMB], bsn = 0.0;
                constexpr int PER_R = NTMB + (SPLIT ? 1 : 0);  // MFMAs per row tile and k-step
                constexpr int SLOTS = RT * PER_R;
                static_for<SLOTS>([&](auto i_tag) {
                    constexpr int i = decltype(i_tag)::value, r = i / PER_R, t = i % PER_R;
                    // am = bit ? 1.0 : 0.0 in two ops: sign-extended 1-bit field (0 / -1) & high word of 1.0
                    const int sh = (((DW * wave) & 127) >> 1) + 8 * r;
                    const int am_hi = __builtin_amdgcn_sbfe((int)(unsigned)(mwc >> (sh & 32)), (sh & 31) + (l15 >> 1), 1) & 0x3FF00000;
                    const double am = __hiloint2double(am_hi, 0);
                    if constexpr (t < NTMB) {
                        accM[r][t] = mfma(am, bwc[t], accM[r][t]);
                    } else {
                        accS[r] = __builtin_amdgcn_mfma_f64_4x4x4f64(am, bsc, accS[r], 0, 0, 0);
                    }
                    if constexpr (s < RPW) {  // the row's pieces spread evenly over the step's MFMAs
                        constexpr int P0 = i * STAGE_PIECES / SLOTS, P1 = (i + 1) * STAGE_PIECES / SLOTS;
                        static_for<P1 - P0>([&](auto o_tag) {
                            stage_piece(tile + 1, lane, s_tag, std::integral_constant<int, P0 + decltype(o_tag)::value>{});
                        });
                    }
                    if constexpr (i == SLOTS * 3 / 4 && s + 1 < 8) {
                        const int smp = 4 * (s + 1) + l4;
                        mwn = Msc[smp * 4 + mword];
#pragma unroll
                        for (int tt = 0; tt < NTMB; ++tt) bwn[tt] = Ws[smp * WS + 16 * tt + l15];
                        if constexpr (SPLIT) bsn = Ws[smp * WS + 16 * NTP + PADS + (lane & 3)];
                    }
                });
                if constexpr (s + 1 < 8) {
                    mwc = mwn;
#pragma unroll
                    for (int t = 0; t < NTMB; ++t) bwc[t] = bwn[t];
                    bsc = bsn;
                }
            });
            stage_end(lane, (int)((tile + 1 - tile_begin) & 1));
#ifdef PPCA_PHASE_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // diagnostic: charge the prefetch wait to P4
#endif
            PPCA_STAMP(7)
        } else if (p.recon) {
            // Output pass on the fp64 MFMA: out (32 samples x 256 dims) = A (32 x kk) . B (kk x 256), wave w owning
            // dims 64 w .. 64 w + 63 (four 16-dim tiles) of both 16-sample row tiles.
            //   smooth / extrapolate (ppca_model.rs:454-463): A = z (K states), B = C^T; + mean
            //   covariance diagonals (:485-508, :542-577): A = vech(Sigma_i) (K' entries), B_j = c_ja c_jb,
            //   doubled off the diagonal (c_j^T Sigma c_j over the packed half); + sigma^2
            // (the scalar form spent 2 K LDS reads per output element, 2 K^2 for the diagonals)
            constexpr int CT = 4;
            const bool dg = p.recon_mode >= 2;
            // Loads and stores share one in-order counter (vmcnt): a load consumed after a store waits for that
            // store to be acknowledged by memory.  So every load of this pass -- the observed values extrapolate
            // passes through bit-exactly -- is issued HERE, before any store of the tile, and the stores at the
            // end run back to back.
            const bool extra = p.recon_mode == 1, zero_obs = p.recon_mode == 3;
            constexpr int ROWS = B / 4;
            double xin[ROWS][4];
#pragma unroll
            for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
                for (int q = 0; q < 4; ++q) xin[rr][q] = 0.0;
            if (extra) {
#pragma unroll
                for (int rr = 0; rr < ROWS; ++rr) {
                    const int64_t row = tile * B + wave + 4 * rr;
                    const double *xrow = p.X + (row < n ? row : n - 1) * p.ldx;
#pragma unroll
                    for (int q = 0; q < 4; ++q) xin[rr][q] = xrow[64 * q + lane < d ? 64 * q + lane : d - 1];
                }
            }
            d4_t oacc[2][CT];
#pragma unroll
            for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
                for (int c4 = 0; c4 < CT; ++c4) oacc[rt2][c4] = d4_t{0, 0, 0, 0};
            const double *crow4[CT];
#pragma unroll
            for (int c4 = 0; c4 < CT; ++c4) crow4[c4] = Cs + (64 * wave + 16 * c4 + l15) * CS;
            if (!dg) {
#pragma unroll
                for (int s = 0; s < (K + 3) / 4; ++s) {
                    const int kx = 4 * s + l4;             // state index of this lane's operands
                    const int ka = kx < K ? kx : K - 1;    // A: any finite value (B is zero there)
                    const int kb = kx < K ? kx : K;        // B: column K of the C tile is all zeros
                    double bo[CT];
#pragma unroll
                    for (int c4 = 0; c4 < CT; ++c4) bo[c4] = crow4[c4][kb];
#pragma unroll
                    for (int rt2 = 0; rt2 < 2; ++rt2) {
                        const double ao = Ws[(16 * rt2 + l15) * WS + ka];
#pragma unroll
                        for (int c4 = 0; c4 < CT; ++c4) oacc[rt2][c4] = mfma(ao, bo[c4], oacc[rt2][c4]);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < (KP + 3) / 4; ++s) {
                    const int e = 4 * s + l4;              // packed index (a >= b) of this lane's operands
                    int ea = 0;
                    while ((ea + 1) * (ea + 2) / 2 <= e) ++ea;
                    int eb = e - ea * (ea + 1) / 2;
                    const double fac = (e < KP) ? (ea == eb ? 1.0 : 2.0) : 0.0;
                    if (e >= KP) { ea = K; eb = K; }       // zero column
                    const int ka = e < KP ? e : KP - 1;
                    double bo[CT];
#pragma unroll
                    for (int c4 = 0; c4 < CT; ++c4) bo[c4] = fac * crow4[c4][ea] * crow4[c4][eb];
#pragma unroll
                    for (int rt2 = 0; rt2 < 2; ++rt2) {
                        const double ao = Ws[(16 * rt2 + l15) * WS + K + ka];
#pragma unroll
                        for (int c4 = 0; c4 < CT; ++c4) oacc[rt2][c4] = mfma(ao, bo[c4], oacc[rt2][c4]);
                    }
                }
            }
            // C/D map of v_mfma_f64_16x16x4: row (sample) = l4 + 4 r, column (dim) = l15.  The results go through
            // the x~ tile (free after P2 in the output passes) and leave as whole rows: per row and wave four
            // 512-byte stores under a wave-uniform row test, the observed values of extrapolate re-read the same
            // way (bit-exact pass-through).  (Storing straight from the accumulator layout put each 8-byte store
            // in its own exec-masked branch with a vmcnt wait: up to 40x slower, depending on hipcc's mood.)
#pragma unroll
            for (int c4 = 0; c4 < CT; ++c4) {
                const double add = dg ? s2 : muo[c4];
#pragma unroll
                for (int rt2 = 0; rt2 < 2; ++rt2)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Xs[(16 * rt2 + l4 + 4 * r) * XS + 64 * wave + 16 * c4 + l15] = oacc[rt2][c4][r] + add;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < ROWS; ++rr) {
                const int ri = wave + 4 * rr;
                const int64_t row = tile * B + ri;
                const bool row_ok = row < n;  // wave-uniform
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = 64 * q + lane;
                    const bool obs = (Msc[ri * 4 + 2 * (q >> 1) + (lane & 1)] >> (32 * (q & 1) + (lane >> 1))) & 1ull;
                    double out = Xs[ri * XS + j];
                    if (extra) out = obs ? xin[rr][q] : out;
                    if (zero_obs) out = obs ? 0.0 : out;
                    if (row_ok && j < d) p.recon[row * (int64_t)d + j] = out;
                }
            }
        }
        __syncthreads();
        PPCA_STAMP(3)
    }
#ifdef PPCA_PHASE_TIMING
    if (p.dbg && tid == 0)
        for (int i = 0; i < 16; ++i) p.dbg[(int64_t)blockIdx.x * 16 + i] = (double)tph[i];
#endif

    // ------------------------------------------------------------ epilogue
    // scalars: deterministic reduction over the 32 solver lanes of each wave, then over the waves
    {
        const double sq_w = wave_sum(lane < SQW ? scl[wave * SQW + lane] : 0.0);
        const double xx_w = wave_sum(xx_run);
        if (lane == 0) {  // xxs is free after the last tile
            xxs[wave] = sq_w;
            xxs[4 + wave] = xx_w;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double v0 = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) v0 += xxs[w];
        double xx_tot = 0.0;  // sum_i w_i |x~_i|^2 (EM pass)
#pragma unroll
        for (int w = 0; w < 4; ++w) xx_tot += xxs[4 + w];
        const int li = lane < B ? lane : 0;
        double sc_llk = scl[L_LLK + li];
        if constexpr (EM) sc_llk -= 0.5 * (log(scl[L_PM + li]) + scl[L_PX + li] * LN_2);
        double v1 = wave_sum(lane < B ? scl[L_DEV + li] : 0.0), v2 = wave_sum(lane < B ? sc_llk : 0.0),
               v3 = wave_sum(lane < B ? scl[L_W + li] : 0.0), v4 = wave_sum(lane < B ? scl[L_NE + li] : 0.0);
        if (lane == 0) {
            double *sc;
            if constexpr (EM) {
                StatsLayout L(d, K);
                sc = p.part + (int64_t)blockIdx.x * L.len + L.scalars;
            } else {
                sc = p.scal_part + (int64_t)blockIdx.x * 8;
            }
            sc[SC_SQERR] = v0;
            sc[SC_DEVSQ] = EM ? v1 + xx_tot : v1;
            sc[SC_LLK] = EM ? v2 - 0.5 * inv_s2 * xx_tot : v2;
            sc[SC_SUMW] = v3;
            sc[SC_NONEMPTY] = v4;
            sc[5] = 0.0;
            sc[6] = 0.0;
            sc[7] = 0.0;
        }
    }
    if constexpr (EM) {
        StatsLayout L(d, K);
        double *out = p.part + (int64_t)blockIdx.x * L.len;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int dim = DW * wave + 16 * r + l4 + 4 * q;  // C/D row of v_mfma_f64_16x16x4
                if (dim >= d) continue;
#pragma unroll
                for (int t = 0; t < NTP; ++t) {
                    const int c = 16 * t + l15;
                    if (c < KP) out[L.S + (int64_t)dim * KP + c] = accM[r][t][q];
                    if constexpr (SPLIT) {  // [w z | w] columns 0 .. PADS-1 sit behind vech(P) in the last tile
                        if (t == NTP - 1 && c >= KP) {
                            const int a = c - KP;
                            if (a < K) out[L.U + (int64_t)dim * K + a] = accM[r][t][q];
                            else if (a == K) out[L.totals + dim] = accM[r][t][q];
                        }
                    }
                }
                if (l15 < K) {
                    if constexpr (!SPLIT) out[L.U + (int64_t)dim * K + l15] = accM[r][NTP][q];
                    out[L.cross + (int64_t)dim * K + l15] = accX[r][q];
                } else if (l15 == K) {
                    if constexpr (!SPLIT) out[L.totals + dim] = accM[r][NTP][q];
                    out[L.sumx + dim] = accX[r][q];
                }
            }
            if constexpr (SPLIT) {  // 4x4x4 group: D lane = 16 i + 4 block + j
                const int dim = DW * wave + 16 * r + 4 * ((lane >> 2) & 3) + (lane >> 4);
                const int a = PADS + (lane & 3);  // index in [w z | w]
                if (dim < d) {
                    if (a < K) out[L.U + (int64_t)dim * K + a] = accS[r];
                    else if (a == K) out[L.totals + dim] = accS[r];
                }
            }
        }
    }
}

template <int K, bool EM, bool GI8>
static hipError_t launch_pass_t(int grid, const PassArgs &a, hipStream_t s) {
    const size_t lds = sizeof(double) * Cfg<K>::LDS_DOUBLES;
    if (hipError_t e = ensure_dynamic_lds<pass_kernel<K, EM, GI8>>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((pass_kernel<K, EM, GI8>), dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

int fused_grid(int64_t n, int n_cu) {
    int64_t tiles = (n + FUSED_TILE - 1) / FUSED_TILE;
    if (tiles < 1) tiles = 1;
    return (int)(tiles < n_cu ? tiles : n_cu);
}

static hipError_t lds_bytes_of(int k, size_t *bytes) {
    PPCA_DISPATCH_K(k, *bytes = sizeof(double) * Cfg<KK>::LDS_DOUBLES);
    return hipSuccess;
}
size_t fused_lds_bytes(int k) {  // 0: a state size the pass is not instantiated for
    size_t bytes = 0;
    return lds_bytes_of(k, &bytes) == hipSuccess ? bytes : 0;
}

// Slice table + guard flags of the current model (device-side, no host sync), then the pass: the int8 variant and,
// behind the guard, the fp64 variant -- each returns at once unless qflag selects it.
template <int K, bool EM>
static hipError_t launch_pass_guarded(int grid, PassArgs a, hipStream_t s) {
    const int mode = fused_gram_mode();
    if (mode == 1) {
        a.qflag = nullptr;
        return launch_pass_t<K, EM, false>(grid, a, s);
    }
    if (!a.skip_qprep) {
        if (hipError_t e = launch_qprep(K, a.model, a.d, a.qscale, a.qtab, a.qflag, s); e != hipSuccess) return e;
    }
    auto int8_pass = [&](const PassArgs &b) {
        if constexpr (!EM) {
            if (!b.states && !b.covs && !b.recon) return launch_llk8(K, grid, b, s);  // llk / llks alone: the eight-wave sweep (ppca_llk.hip)
            if (recon8_covers(b)) return launch_recon8(K, grid, b, s);  // smooth / extrapolate on the same sweep (round 6)
        }
        if constexpr (EM) return launch_em9(K, grid, b, s);  // eight waves, two roles, the solve pipelined across tiles (ppca_em9.hip)
        else return launch_pass_t<K, EM, true>(grid, b, s);
    };
    if (mode == 2) {
        a.qflag = nullptr;
        return int8_pass(a);
    }
    if (hipError_t e = int8_pass(a); e != hipSuccess) return e;
    if constexpr (EM) return hipSuccess;  // the fp64 variant of an EM pass runs behind launch_em_wguard, after the reduction
    return launch_pass_t<K, EM, false>(grid, a, s);
}

hipError_t launch_pass_em(int k, int grid, const PassArgs &a, hipStream_t s) {
    PPCA_DISPATCH_K(k, return (launch_pass_guarded<KK, true>(grid, a, s)));
    return hipErrorInvalidValue;
}

hipError_t launch_pass_post(int k, int grid, const PassArgs &a, hipStream_t s) {
    PPCA_DISPATCH_K(k, return (launch_pass_guarded<KK, false>(grid, a, s)));
    return hipErrorInvalidValue;
}
hipError_t launch_pass_post_fp64(int k, int grid, const PassArgs &a, hipStream_t s) {
    PPCA_DISPATCH_K(k, return (launch_pass_t<KK, false, false>(grid, a, s)));
    return hipErrorInvalidValue;
}
hipError_t launch_em_fallback(int k, int grid, PassArgs a, const GuardArgs &g, const double *part, double *part2, int64_t len, double *stats,
                              hipStream_t s) {
    a.runflag = g.qflag + QF_MODE;
    a.who = g.who;
    a.part = part2;
    a.errb = nullptr;
    PPCA_DISPATCH_K(k, {
        if (hipError_t e = launch_pass_t<KK, true, false>(grid, a, s); e != hipSuccess) return e;
    });
    return launch_reduce_fallback(part, part2, g, len, stats, s);
}

}  // namespace ppca
