// batch_quality_kernels.hip — what a batch reads and writes for all its items at once in FLAT launches, whose workgroups
// find their item in a per-workgroup table (batch_readout_plan.h builds it; read as K1f reads block_item, never searched):
//   K4c / K6c  packed layout coordinates of every item, up or down (reorder_positions_kernel, index_kernels.hip, per item)
//   K7g        K7a's figures of every item for a list of step distances (pair_errors_kernel, quality_kernels.hip, per item)
// The kernels write the planes of the items (K4c), or their own output buffers only (K6c, K7g).  No floating-point atomics.
#include "sgd_host.h"
#include "quality_device.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// ---- K4c / K6c ---------------------------------------------------------------------------------------
// Workgroup b moves COORD_BLOCK consecutive words of item block_item[b]; thread t of the item's local numbering walks the
// packed ABI order, word t = (k*2 + end)*D + dim of dense node k, as reorder_positions_kernel does: the packed side is one
// coalesced run per workgroup, the plane side a gather (down) or scatter (up) of x[(end*D + dim)*n + perm[k]].  A word is
// copied as it is: every bit pattern of a double survives.
__global__ void __launch_bounds__(COORD_BLOCK) batch_coords_kernel(const CoordItem *items, const uint32_t *block_item, double *packed,
                                                                   const int to_device) {
    const CoordItem it = items[block_item[blockIdx.x]];
    const uint64_t W = 2ull * it.dims, words = (uint64_t)it.n * W;
    const uint64_t t = (uint64_t)(blockIdx.x - it.first_block) * COORD_BLOCK + threadIdx.x;
    if (t >= words) return;
    const uint64_t k = t / W, r = t - k * W;                               // r = end*D + dim
    const uint64_t dev = r * it.n + it.perm[k];
    if (to_device) it.x[dev] = packed[it.offset + t]; else packed[it.offset + t] = it.x[dev];
}

hipError_t batch_coords_device(const CoordItem *d_items, const uint32_t *d_block_item, uint64_t blocks, double *d_packed, int to_device,
                               hipStream_t st) {
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;               // a grid's x dimension
    hipLaunchKernelGGL(batch_coords_kernel, dim3((unsigned)blocks), dim3(COORD_BLOCK), 0, st, d_items, d_block_item, d_packed, to_device);
    return hipGetLastError();
}

// ---- K7g ---------------------------------------------------------------------------------------------
// grid (sum of the items' quality_blocks, n_z).  Workgroup b of a row is local block b - first_block of its item, in a local
// grid of the item's own quality_blocks(n_steps) workgroups: a thread starts at local_block * Q_BLOCK + threadIdx.x and strides
// by blocks * Q_BLOCK, which is exactly the list of pairs pair_errors_kernel gives the thread of that block in the item's own
// launch, in the same order; the per-pair function and the workgroup's reduction are the same text (quality_device.h).  The
// partials of a row lie in workgroup order, an item's side by side, and the reduce below — one workgroup per (item, z) —
// sums an item's partials from zero in that order, as reduce_partials_kernel sums the item's own launch.  Same values, same
// order, same operations: the figures are gfs_ctx_pair_errors' bit for bit, whatever else is in the batch.
__global__ void __launch_bounds__(Q_BLOCK) batch_pair_errors_kernel(const QualityItem *items, const uint32_t *block_item, const uint32_t dims,
                                                                    const uint64_t *zs, uint64_t *partials) {
    const QualityItem it = items[block_item[blockIdx.x]];
    const uint32_t zi = blockIdx.y;
    const uint64_t z = zs[zi];
    uint64_t pairs = 0;
    double sum_rel = 0.0, max_rel = 0.0, sum_abs = 0.0, sum_sq = 0.0;
    if (z < it.n_steps) {
        const uint64_t n = it.n_steps - z, stride = (uint64_t)it.blocks * Q_BLOCK;
        for (uint64_t s = (uint64_t)(blockIdx.x - it.first_block) * Q_BLOCK + threadIdx.x; s < n; s += stride) {
            double err, rel;
            if (!pair_error(it.step_rec[s], it.step_rec[s + z], it.x, it.n_nodes, dims, err, rel)) continue;
            ++pairs;
            sum_rel += rel;
            max_rel = rel > max_rel ? rel : max_rel;
            sum_abs += fabs(err);
            sum_sq += err * err;
        }
    }
    uint64_t v[5] = {pairs, (uint64_t)__double_as_longlong(sum_rel), (uint64_t)__double_as_longlong(max_rel),
                     (uint64_t)__double_as_longlong(sum_abs), (uint64_t)__double_as_longlong(sum_sq)};
    store_block_partials<PairFields>(v, partials, gridDim.y, zi);
}

// partials[field][zi][first_block .. first_block + blocks) of item blockIdx.x -> out[item][zi][field], summed in workgroup
// order by thread 0 (reduce_item_partials, quality_device.h: reduce_partials_kernel's loop).  grid (items, n_z).
__global__ void __launch_bounds__(Q_BLOCK) batch_reduce_partials_kernel(const QualityItem *items, const uint64_t *partials, const uint32_t row_blocks,
                                                                        uint64_t *out) {
    const QualityItem it = items[blockIdx.x];
    reduce_item_partials<PairFields>(partials, gridDim.y, blockIdx.y, row_blocks, it.first_block, it.blocks,
                                     out + ((uint64_t)blockIdx.x * gridDim.y + blockIdx.y) * 5);
}

hipError_t batch_pair_errors_device(const QualityItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks,
                                    uint32_t dims, const uint64_t *d_zs, uint32_t n_z, uint64_t *d_partials, uint64_t *d_out, hipStream_t st) {
    if (n_z == 0 || n_items == 0) return hipSuccess;
    if (row_blocks == 0 || row_blocks > 0x7FFFFFFFull || n_z > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_pair_errors_kernel, dim3((unsigned)row_blocks, n_z), dim3(Q_BLOCK), 0, st, d_items, d_block_item, dims, d_zs, d_partials);
    hipLaunchKernelGGL(batch_reduce_partials_kernel, dim3(n_items, n_z), dim3(Q_BLOCK), 0, st, d_items, d_partials, (uint32_t)row_blocks, d_out);
    return hipGetLastError();
}

}  // namespace gfs
