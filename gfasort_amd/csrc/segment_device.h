// segment_device.h — what ONE workgroup does with ONE item's segment in LDS, shared by K4b / K6b (batch_readout_kernels.hip) and
// K7k (batch_sort_quality_kernels.hip): the bitonic network over (key, dense index) pairs, and the exclusive scan of one chunk of
// blockDim.x 64-bit values.  One text for both units, so that K7k's rank order is K6b's and its prefix sums are K4b's.
// The network's arithmetic is segment_sort.h's, which the host runs serially in its tests.
#pragma once
#include "segment_sort.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// keys[0..P), index[0..P) in LDS, filled (padding included) and visible to the workgroup (a barrier behind the last write); P a
// power of two >= 64, B = blockDim.x = segment_block(P), so every thread is live in every loop below.  Element t of the segment is
// held by thread t % B: a partner at distance j < 64 is lane ^ j of the same wave, and those stages run in registers over wave
// shuffles, a chunk of B elements at a time; the stages with j >= 64 exchange through LDS, consecutive lanes on consecutive 8-byte
// keys (no bank conflict), with a barrier each.  P = 8192: 28 LDS stages and 13 wave passes for 91 stages.  Ends behind a barrier.
__device__ __forceinline__ void segment_network(uint64_t *keys, uint32_t *index, const uint32_t P, const uint32_t B, const uint32_t tid) {
    for (uint32_t k = 2; k <= P; k <<= 1) {
        uint32_t j = k >> 1;
        for (; j >= SEGMENT_WAVE; j >>= 1) {
            for (uint32_t q = tid; q < P / 2; q += B) {
                const uint32_t lo = segment_pair_low(q, j), hi = segment_partner(lo, j);
                const uint64_t k_lo = keys[lo], k_hi = keys[hi];
                const uint32_t i_lo = index[lo], i_hi = index[hi];
                if (segment_takes_other(lo, k, j, k_lo, i_lo, k_hi, i_hi)) {
                    keys[lo] = k_hi; keys[hi] = k_lo;
                    index[lo] = i_hi; index[hi] = i_lo;
                }
            }
            __syncthreads();
        }
        const uint32_t j_wave = j;                                          // min(k / 2, 32)
        for (uint32_t t = tid; t < P; t += B) {                            // (P and B are multiples of 64: whole waves)
            uint64_t key = keys[t];
            uint32_t idx = index[t];
            for (j = j_wave; j >= 1; j >>= 1) {
                const uint64_t k_other = __shfl_xor((unsigned long long)key, (int)j);
                const uint32_t i_other = __shfl_xor(idx, (int)j);
                if (segment_takes_other(t, k, j, key, idx, k_other, i_other)) { key = k_other; idx = i_other; }
            }
            keys[t] = key; index[t] = idx;
        }
        __syncthreads();
    }
}

// One chunk of blockDim.x values, `len` being this thread's: an inclusive scan over the wave by shuffles, the waves' totals through
// wave_total[0..n_waves) (LDS), n_waves = blockDim.x / 64 <= 16.  Returns the sum of the values of the threads before this one;
// total = the chunk's sum (the same in every thread).  Every thread of the workgroup calls it (two barriers: wave_total is free
// again on return).  Integer arithmetic: the result does not depend on the launch shape.
__device__ __forceinline__ uint64_t block_scan_chunk(const uint64_t len, uint64_t *wave_total, const uint32_t n_waves, uint64_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t incl = len;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < n_waves; ++w) {
        const uint64_t s = wave_total[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();
    return before + incl - len;
}

}  // namespace gfs
