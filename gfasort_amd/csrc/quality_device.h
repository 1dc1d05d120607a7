// quality_device.h — the device functions K7 (quality_kernels.hip) and K7g (batch_quality_kernels.hip) share: the one per-pair
// function and the fixed-tree reduction of a workgroup's five fields.  One text for both units, so that a batch's figures
// are the per-item call's bit for bit.
#pragma once
#include "batch_readout_plan.h"                           // Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

static constexpr uint32_t Q_NO_NODE = 0xFFFFFFFFu;

// ---- the one per-pair function (sgd.rs:1252-1275) ---------------------------------------------------------------------
// step record: { slot | NO_NODE, path | rev << 31, pos lo, pos hi (23 bits) | crowding exponents } (index_kernels.hip)
__device__ __forceinline__ uint64_t rec_pos(const uint4 r) { return (uint64_t)r.z | ((uint64_t)(r.w & 0x7FFFFFu) << 32); }
__device__ __forceinline__ uint32_t rec_path(const uint4 r) { return r.y & 0x7FFFFFFFu; }

// x: the context's position buffer in its own order — 1D x[slot] (dims = 0), nD the planes [end][dim][slot], of which the
// '+' end (end 0) is planes 0..dims-1.  False: the pair is skipped (another path, d_path == 0, an absent node).
__device__ __forceinline__ bool pair_error(const uint4 ra, const uint4 rb, const double *x, const uint64_t n_nodes, const uint32_t dims,
                                           double &err, double &rel_sq) {
    if (rec_path(ra) != rec_path(rb)) return false;
    const double d_path = fabs((double)rec_pos(ra) - (double)rec_pos(rb));   // :1252-1254
    if (d_path == 0.0) return false;                                         // :1256
    if (ra.x == Q_NO_NODE || rb.x == Q_NO_NODE) return false;                // :1260-1267
    double sum_sq = 0.0;                                                     // layout.rs:126-133
    const uint32_t terms = dims ? dims : 1u;
    for (uint32_t d = 0; d < terms; ++d) {
        const double delta = x[(uint64_t)d * n_nodes + ra.x] - x[(uint64_t)d * n_nodes + rb.x];
        sum_sq += delta * delta;
    }
    err = sqrt(sum_sq) - d_path;                                             // :1273
    rel_sq = (err * err) / (d_path * d_path);                                // :1274
    return true;
}

// ---- fixed-tree reductions ------------------------------------------------------------------------------------------------
// Five 8-byte fields per accumulator; what a field is says how it is combined.
enum FieldOp { SUM_U64, SUM_F64, MAX_F64 };
struct PairFields {                                                        // pairs, sum_rel_sq, max_rel_sq, sum_abs, sum_sq
    static __host__ __device__ constexpr FieldOp op(int f) { return f == 0 ? SUM_U64 : f == 2 ? MAX_F64 : SUM_F64; }
};
struct SortFields {                                                        // steps, abs_err_sum, genomic_sum, sq_err_sum, -
    static __host__ __device__ constexpr FieldOp op(int f) { return f == 3 ? SUM_F64 : SUM_U64; }
};

__device__ __forceinline__ uint64_t combine(const FieldOp op, const uint64_t a, const uint64_t b) {
    if (op == SUM_U64) return a + b;
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return (uint64_t)__double_as_longlong(op == SUM_F64 ? x + y : (y > x ? y : x));
}

// One workgroup's five fields -> partials[field][zi][block].  Butterfly over the wave (both partners of a step compute the
// same commutative a + b), then thread 0 combines the waves in wave order.
template <typename F>
__device__ __forceinline__ void store_block_partials(uint64_t (&v)[5], uint64_t *partials, const uint32_t n_z, const uint32_t zi) {
    __shared__ uint64_t wave_part[Q_BLOCK / 64][5];
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            v[f] = combine(F::op(f), v[f], (uint64_t)__shfl_xor((unsigned long long)v[f], off, 64));
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int f = 0; f < 5; ++f) wave_part[wave][f] = v[f];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            uint64_t t = wave_part[0][f];
            for (unsigned w = 1; w < Q_BLOCK / 64; ++w) t = combine(F::op(f), t, wave_part[w][f]);
            partials[((uint64_t)f * n_z + zi) * gridDim.x + blockIdx.x] = t;
        }
    }
}

}  // namespace gfs
