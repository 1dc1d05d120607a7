// batch_readout_kernels.hip — what a batch does either side of its SGD launch, for all its items at once, one workgroup per item:
//   K4b  initial positions of every item (K4, index_kernels.hip, without its rocPRIM scans and allocations)
//   K6b  positions in dense order and rank order of every item (K6 without its radix passes): a graph of a few thousand nodes
//        fits in one workgroup's LDS, where a bitonic network sorts its (key, dense index) pairs
// The network's arithmetic is segment_sort.h's, which the host runs serially in its tests; what a workgroup does with it, and the
// scan of a chunk, are segment_device.h's.
#include "sgd_host.h"
#include "segment_sort.h"
#include "segment_device.h"
#include "sort_key.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// ---- K6b -----------------------------------------------------------------------------------------
// Workgroup b sorts item items[b]; all items of a launch have the same padded length P (the launch's LDS: P keys, then P
// indices) and the block is segment_block(P).  The network itself is segment_device.h's segment_network, which K7k shares.
__global__ void __launch_bounds__(1024) segment_sort_kernel(const ReadoutItem *items, double *positions, uint32_t *order) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ReadoutItem it = items[blockIdx.x];
    const uint32_t n = it.n, P = it.padded, B = blockDim.x, tid = threadIdx.x;
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem);
    uint32_t *index = reinterpret_cast<uint32_t *>(keys + P);
    for (uint32_t t = tid; t < P; t += B) {
        uint64_t key = SEGMENT_PAD_KEY;
        uint32_t idx = SEGMENT_PAD_INDEX;
        if (t < n) {
            const double v = it.x[it.perm[t]];
            if (positions) positions[it.offset + t] = v;                   // ABI dense order (gfs_ctx_download_positions)
            key = orderable(v); idx = t;
        }
        keys[t] = key; index[t] = idx;
    }
    __syncthreads();
    segment_network(keys, index, P, B, tid);
    for (uint32_t t = tid; t < n; t += B) order[it.offset + t] = index[t];
}

hipError_t sort_segments_device(const ReadoutItem *d_items, uint32_t count, uint32_t padded, double *d_positions, uint32_t *d_order,
                                hipStream_t st) {
    if (count == 0) return hipSuccess;
    if (padded < SEGMENT_WAVE || (padded & (padded - 1)) || padded > SEGMENT_SORT_CAP) return hipErrorInvalidValue;
    const size_t lds = (size_t)segment_lds_bytes(padded);
    if (lds > 64u * 1024u) {                                               // beyond the default limit of a launch's dynamic LDS
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&segment_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)segment_lds_bytes(SEGMENT_SORT_CAP));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(segment_sort_kernel, dim3(count), dim3(segment_block(padded)), lds, st, d_items, d_positions, d_order);
    return hipGetLastError();
}

// ---- K4b -----------------------------------------------------------------------------------------
// x[perm[k]] = sum of node_len[0 .. k) (sgd.rs:286-294) for item items[blockIdx.x]: chunks of one block, an inclusive scan over the
// wave by shuffles, the waves' totals through LDS (segment_device.h block_scan_chunk, which K7k shares), the running sum carried
// from chunk to chunk.  Integer arithmetic: the result does not depend on the launch shape.
constexpr uint32_t INIT_BLOCK = 256;
__global__ void __launch_bounds__(INIT_BLOCK) batch_init_positions_kernel(const ReadoutItem *items) {
    __shared__ uint64_t wave_total[INIT_BLOCK / 64];
    const ReadoutItem it = items[blockIdx.x];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < it.n; base += INIT_BLOCK) {             // (the same trips for every thread)
        const uint64_t k = base + threadIdx.x;
        const uint64_t len = k < it.n ? (uint64_t)it.node_len[k] : 0ull;
        uint64_t total;
        const uint64_t before = block_scan_chunk(len, wave_total, INIT_BLOCK / 64, total);
        if (k < it.n) it.x[it.perm[k]] = (double)(carry + before);         // the reference accumulates in usize and converts (sgd.rs:291)
        carry += total;
    }
}

hipError_t batch_init_positions_device(const ReadoutItem *d_items, uint32_t count, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_init_positions_kernel, dim3(count), dim3(INIT_BLOCK), 0, st, d_items);
    return hipGetLastError();
}

}  // namespace gfs
