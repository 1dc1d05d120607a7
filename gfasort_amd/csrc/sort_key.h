// sort_key.h — the sort key of a position, shared by K6 (index_kernels.hip) and K6b (batch_readout_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// Order-preserving u64 image of an f64: -0.0 is folded onto +0.0 (partial_cmp calls them equal, so the
// tie must be broken by index, sgd.rs:666); NaNs (never produced by a finite run) sort after all numbers.
__device__ __forceinline__ uint64_t orderable(double v) {
    if (v != v) return 0xFFFFFFFFFFFFFFFFull;
    if (v == 0.0) v = 0.0;
    uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

}  // namespace gfs
