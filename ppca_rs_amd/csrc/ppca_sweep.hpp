// ppca_sweep.hpp -- what the streaming sweeps (ppca_scale.hip, ppca_heldout.hip, ppca_kmeans.hip) and the row-wise passes
// (ppca_sample.hip, ppca_loo.hip, ppca_heldout.hip, the synthetic data of ppca_util.hip) share, each defined here and nowhere else:
// the counter-based generator and every stream id of the library, the 16-byte column-pair access and the launchers' choice of it, a
// workgroup's cut of a sweep, and the constants of the per-entry predictives.  DESIGN.md section 4.18.  Not installed.
#pragma once

#include <initializer_list>

#include "ppca_device.hpp"

namespace ppca {

// ------------------------------------------------------------------ the generator
// Every stream of the library: draws are keyed by (seed, stream, global row, index), and two streams never meet as long as every id
// is given out here.  smix64, row_key, row_word and u01_floor are host code too: the host-side split of row-compressed data
// (ppca_sparse_heldout.hip, ppca_heldout_split_csr_host) draws the words of holdout_kernel.
enum RngStream : uint64_t {
    STREAM_SYNTH_LATENT = 1,  // synthetic data: z
    STREAM_SYNTH_NOISE = 2,   //   the noise of x
    STREAM_SYNTH_MASK = 3,    //   the Bernoulli mask
    STREAM_SYNTH_RUN = 4,     //   the start of a row's masked run
    STREAM_EPS = 5,           // posterior sampling: eps (k normals)
    STREAM_ETA = 6,           //   eta (d normals)
    STREAM_CHOICE = 7,        //   the mixture's component of a row
    STREAM_HOLDOUT = 8,       // the hold-out split
};

__host__ __device__ __forceinline__ uint64_t smix64(uint64_t x) {  // splitmix64's finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// once per row and stream
__host__ __device__ __forceinline__ uint64_t row_key(uint64_t seed, uint64_t stream, uint64_t grow) {
    return smix64(smix64(seed ^ (stream * 0xD1342543DE82EF95ull)) + grow);
}
// word p of a row's stream
__host__ __device__ __forceinline__ uint64_t row_word(uint64_t key, uint64_t p) { return smix64(key + p * 0xA0761D6478BD642Full); }
// The two uniforms in use, from the top 53 bits of a word.  They are different draws: which one a stream takes is part of it.
__host__ __device__ __forceinline__ double u01_floor(uint64_t w) { return (double)(w >> 11) * (1.0 / 9007199254740992.0); }         // [0, 1)
__device__ __forceinline__ double u01_open(uint64_t w) { return ((double)(w >> 11) + 0.5) * (1.0 / 9007199254740992.0); }  // (0, 1)

// ------------------------------------------------------------------ 16-byte column pairs
typedef double d2_t __attribute__((ext_vector_type(2)));

template <int VEC>
struct Vec {
    double v[VEC];
};

// NT: non-temporal access.  A sweep touches every byte once; measured at 4 M x 256 and 1 M x 1024 scale_kernel is 2 %
// faster with the output and 8-10 % faster in the sums-only form than with plain loads and stores.
template <int VEC, bool NT>
__device__ __forceinline__ Vec<VEC> load_vec(const double *p) {
    Vec<VEC> r;
    if constexpr (VEC == 2) {
        const d2_t t = NT ? __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(p)) : *reinterpret_cast<const d2_t *>(p);
        r.v[0] = t.x;
        r.v[1] = t.y;
    } else {
        r.v[0] = NT ? __builtin_nontemporal_load(p) : *p;
    }
    return r;
}
template <int VEC, bool NT>
__device__ __forceinline__ void store_vec(double *p, const Vec<VEC> &r) {
    if constexpr (VEC == 2) {
        d2_t t;
        t.x = r.v[0];
        t.y = r.v[1];
        if (NT)
            __builtin_nontemporal_store(t, reinterpret_cast<d2_t *>(p));
        else
            *reinterpret_cast<d2_t *>(p) = t;
    } else {
        if (NT)
            __builtin_nontemporal_store(r.v[0], p);
        else
            *p = r.v[0];
    }
}

// Threads per row of a sweep: the power of two that covers the row's slots, at most 256.
inline int sweep_tpr_log2(int slots) {
    int lg = 0;
    while ((1 << lg) < slots && lg < 8) ++lg;
    return lg;
}

// A launcher's choice: column pairs when d and the row strides are even and every pointer (null counts as aligned) is 16-byte aligned,
// single columns otherwise; the slots of a row; the threads per row.
struct SweepCut {
    bool vec;
    int slots, tpr_log2;
};
inline SweepCut sweep_cut(int d, bool even_strides, std::initializer_list<const void *> ptrs) {
    bool vec = d % 2 == 0 && even_strides;
    for (const void *p : ptrs) vec = vec && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const int slots = vec ? d / 2 : d;
    return {vec, slots, sweep_tpr_log2(slots)};
}

// ------------------------------------------------------------------ a workgroup's cut of a sweep
// THREADS threads as (rows per step rps) x (threads per row tpr): thread t is column tc of row group tr; a row has `slots` slots of
// VEC columns; the workgroup takes rows r0 .. r1 of n.  By reference, in this order: returned as a struct they changed holdout_kernel.
template <int THREADS, int VEC>
__device__ __forceinline__ void sweep_layout(int t, int d, int tpr_log2, int64_t rows_per_wg, int64_t n, int &tpr, int &rps, int &tc,
                                             int &tr, int &slots, int64_t &r0, int64_t &r1) {
    tpr = 1 << tpr_log2, rps = THREADS >> tpr_log2;
    tc = t & (tpr - 1), tr = t >> tpr_log2;
    slots = (d + VEC - 1) / VEC;
    r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
}

// NOT here, because as inlined routines they changed their kernels' code (profiles/shared_sweep): the sweeps' fixed-order column sum
// through red[], and the predictives' blocked loop for c_j^T Sigma c_j, staging of Sigma and z, and log-sum-exp push.

// ------------------------------------------------------------------ the per-entry predictives (ppca_loo.hip, ppca_heldout.hip)
// ln 2 pi as these two files have always spelt it: 0x1.d67f1c864beb5p+0.  LN_2PI of ppca_small.hpp (1.8378770664093453) is
// 0x1.d67f1c864beb4p+0, one ulp below.  Both stay: either one in the other's place changes the last bit of every log-density it enters.
constexpr double LOG_2PI = 1.8378770664093454836;

__host__ __device__ inline int pad16(int k) { return (k + 15) / 16 * 16; }

}  // namespace ppca
