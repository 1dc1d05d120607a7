// batch_sort_quality_kernels.hip — K7k: K7c (gfs_ctx_sort_quality, quality_kernels.hip) of every item of a batch of 1D sorts, in a
// number of launches that does not depend on the number of items:
//   a  sorted positions: one workgroup per item sorts the item's (key, dense index) pairs in LDS (K6b's network), scans the node
//      lengths in rank order (K4b's scan) and writes the sorted position of every node, by slot, into a packed array
//   b  the step pass over K7g's block plan: K7c's pairs, thread for thread, on the item's own tables
//   c  the reduce: one workgroup per item sums the item's partials from zero in workgroup order
// Network, scan, per-pair loop, workgroup reduction and the sum of partials are the texts K6b, K4b and K7c run (segment_device.h,
// quality_device.h): same values, same order, same operations — an item's row is gfs_ctx_sort_quality's bit for bit, whatever
// else is in the batch.  The kernels write their own output buffers only.  No floating-point atomics.
#include "sgd_host.h"
#include "segment_sort.h"
#include "segment_device.h"
#include "sort_key.h"
#include "quality_device.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// ---- a ---------------------------------------------------------------------------------------------
// Workgroup b works on item items[b]; all items of a launch have the same padded length P (the launch's LDS: P keys, then P
// indices) and the block is segment_block(P), as in K6b.  After the network index[r] is the dense index of the node of rank r:
// prefix[r] = the lengths of the nodes of rank < r (measure_layout_quality.rs:100-127), in chunks of one block, the running sum
// carried from chunk to chunk.  The keys are dead after the sort: the waves' totals of a chunk go to their first 16 words, so the
// launch's LDS stays segment_lds_bytes(P), all of it dynamic.  spos[offset + perm[index[r]]] = prefix[r] — by slot, as
// scatter_sorted_pos_kernel writes it; totals[b] = the item's length in bp.  A thread reads index[r] for r = tid + chunk * B only,
// which the network's last barrier made visible, and writes nothing into index.
__global__ void __launch_bounds__(1024) batch_sorted_positions_kernel(const ReadoutItem *items, uint64_t *spos, uint64_t *totals) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ReadoutItem it = items[blockIdx.x];
    const uint32_t n = it.n, P = it.padded, B = blockDim.x, tid = threadIdx.x;
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem);
    uint32_t *index = reinterpret_cast<uint32_t *>(keys + P);
    for (uint32_t t = tid; t < P; t += B) {
        uint64_t key = SEGMENT_PAD_KEY;
        uint32_t idx = SEGMENT_PAD_INDEX;
        if (t < n) { key = orderable(it.x[it.perm[t]]); idx = t; }
        keys[t] = key; index[t] = idx;
    }
    __syncthreads();
    segment_network(keys, index, P, B, tid);
    uint64_t *wave_total = keys;                                           // (P >= 64 words; a block has at most 16 waves)
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n; base += B) {                         // (the same trips for every thread)
        const uint32_t r = base + tid;
        const uint32_t k = r < n ? index[r] : 0u;
        const uint64_t len = r < n ? (uint64_t)it.node_len[k] : 0ull;
        uint64_t total;
        const uint64_t before = block_scan_chunk(len, wave_total, B >> 6, total);
        if (r < n) spos[it.offset + it.perm[k]] = carry + before;
        carry += total;
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

hipError_t batch_sorted_positions_device(const ReadoutItem *d_items, uint32_t count, uint32_t padded, uint64_t *d_spos, uint64_t *d_totals,
                                         hipStream_t st) {
    if (count == 0) return hipSuccess;
    if (padded < SEGMENT_WAVE || (padded & (padded - 1)) || padded > SEGMENT_SORT_CAP) return hipErrorInvalidValue;
    const size_t lds = (size_t)segment_lds_bytes(padded);
    if (lds > 64u * 1024u) {                                               // beyond the default limit of a launch's dynamic LDS
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&batch_sorted_positions_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)segment_lds_bytes(SEGMENT_SORT_CAP));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(batch_sorted_positions_kernel, dim3(count), dim3(segment_block(padded)), lds, st, d_items, d_spos, d_totals);
    return hipGetLastError();
}

// ---- b ---------------------------------------------------------------------------------------------
// grid: the sum of the items' quality_blocks.  Workgroup b is local block b - first_block of its item, in a local grid of the
// item's own quality_blocks(n_steps) workgroups: a thread starts at local_block * Q_BLOCK + threadIdx.x and strides by blocks *
// Q_BLOCK — the very pairs, in the very order, that sort_quality_kernel gives the thread of that block in the item's own launch.
// The partials lie in workgroup order, [field][workgroup of the row], an item's side by side.
__global__ void __launch_bounds__(Q_BLOCK) batch_sort_quality_kernel(const SortQualityItem *items, const uint32_t *block_item, uint64_t *partials) {
    const SortQualityItem it = items[block_item[blockIdx.x]];
    uint64_t steps = 0, abs_sum = 0, gen_sum = 0;
    double sq_sum = 0.0;
    sort_quality_pairs(it.step_rec, it.n_steps, it.spos, blockIdx.x - it.first_block, it.blocks, steps, abs_sum, gen_sum, sq_sum);
    uint64_t v[5] = {steps, abs_sum, gen_sum, (uint64_t)__double_as_longlong(sq_sum), 0};
    store_block_partials<SortFields>(v, partials, 1, 0);
}

// ---- c ---------------------------------------------------------------------------------------------
// out[item][0..5) = { steps, abs_err_sum, genomic_sum (u64), sq_err_sum (f64 bits), 0 }: reduce_partials_kernel<SortFields>'s sum
// over the item's own workgroups.  grid: items.
__global__ void __launch_bounds__(Q_BLOCK) batch_sort_quality_reduce_kernel(const SortQualityItem *items, const uint64_t *partials,
                                                                            const uint32_t row_blocks, uint64_t *out) {
    const SortQualityItem it = items[blockIdx.x];
    reduce_item_partials<SortFields>(partials, 1, 0, row_blocks, it.first_block, it.blocks, out + (uint64_t)blockIdx.x * 5);
}

hipError_t batch_sort_quality_device(const SortQualityItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks,
                                     uint64_t *d_partials, uint64_t *d_out, hipStream_t st) {
    if (n_items == 0) return hipSuccess;
    if (row_blocks == 0 || row_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;   // a grid's x dimension
    hipLaunchKernelGGL(batch_sort_quality_kernel, dim3((unsigned)row_blocks), dim3(Q_BLOCK), 0, st, d_items, d_block_item, d_partials);
    hipLaunchKernelGGL(batch_sort_quality_reduce_kernel, dim3(n_items), dim3(Q_BLOCK), 0, st, d_items, d_partials, (uint32_t)row_blocks, d_out);
    return hipGetLastError();
}

}  // namespace gfs
