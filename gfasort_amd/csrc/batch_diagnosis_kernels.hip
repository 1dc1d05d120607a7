// batch_diagnosis_kernels.hip — K7d / K7e / K7f (quality_kernels.hip) for every item of a batch at once, in launches whose
// number does not depend on the number of items:
//   K7h  per path: the tiles of all items are one FLAT tile space (batch_readout_plan.h tile_plan); a wave reads its tile's item
//        from a table and runs K7d's tile body on the item's own step table with the LOCAL tile index; one wave per path of the
//        union folds that path's tiles
//   K7i  the stretched pairs: counts per flat tile, ONE exclusive scan over all of them, an ordered write per item
//   K7j  per node: K7f's atomics over K7g's block plan into a packed slot array, one gather through every item's node layout
// What a wave does with a tile, a path or a pair is quality_device.h's text, the one K7d-f run: a tile's yield does not depend on
// the grid that ran it, a path's tiles are folded in tile order, per node only integer sums and a maximum are accumulated — so
// item i's rows are, bit for bit, those of its own gfs_ctx_* call, whatever else is in the batch.  No LDS, no barrier; the only
// atomics are K7f's.  The kernels read the items' tables and positions and write only the buffers handed to them.
#include "sgd_host.h"
#include "quality_device.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>

namespace gfs {

// the item that owns union index v of the kind `first` counts: the last i with items[i].*first <= v (items without any share
// a boundary with their successor: take the last).  The table is small and stays in cache.
__device__ __forceinline__ uint32_t diag_item_of(const DiagItem *items, const uint32_t n_items, const uint64_t v, uint64_t DiagItem::*first) {
    uint32_t lo = 0, hi = n_items;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (items[mid].*first <= v) lo = mid; else hi = mid; }
    return lo;
}
// a value every lane of the wave holds, as the scalar it is: what is loaded through it is loaded once per wave
__device__ __forceinline__ uint32_t wave_uniform(const uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

static unsigned wave_grid(uint64_t waves, uint64_t max_blocks) {
    const uint64_t cap = max_blocks && max_blocks < Q_TILE_MAX_BLOCKS ? max_blocks : Q_TILE_MAX_BLOCKS;
    const uint64_t b = (waves + Q_BLOCK / 64 - 1) / (Q_BLOCK / 64);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- K7h ------------------------------------------------------------------------------------------------------------------
// head, tail: 5 words per flat tile, an item's at first_tile * 5, so that local tile t lies at (first_tile + t) * 5; out: 8 words
// per path of the union, an item's at first_path * 8.  Neighbouring waves of a workgroup may work for different items.
__global__ void __launch_bounds__(Q_BLOCK) batch_path_tiles_kernel(const DiagItem *__restrict__ items, const uint32_t *__restrict__ tile_item, const uint32_t dims,
                                                                   const uint64_t z, const double ratio, const uint64_t n_tiles, uint64_t *head,
                                                                   uint64_t *tail, uint64_t *out) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; t < n_tiles; t += (uint64_t)gridDim.x * (Q_BLOCK / 64)) {
        const DiagItem it = items[wave_uniform(tile_item[t])];
        path_tile(it.step_rec, it.n_steps, it.x, it.n_nodes, dims, z, ratio, t - it.first_tile, lane, head + it.first_tile * 5,
                  tail + it.first_tile * 5, out + it.first_path * 8);
    }
}
__global__ void __launch_bounds__(Q_BLOCK) batch_path_combine_kernel(const DiagItem *__restrict__ items, const uint32_t n_items, const uint64_t n_paths,
                                                                     const uint64_t *head, const uint64_t *tail, uint64_t *out) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t p = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; p < n_paths; p += (uint64_t)gridDim.x * (Q_BLOCK / 64)) {
        const DiagItem it = items[wave_uniform(diag_item_of(items, n_items, p, &DiagItem::first_path))];
        const uint64_t local = p - it.first_path;
        path_fold(it.path_rec[local], local, lane, head + it.first_tile * 5, tail + it.first_tile * 5, out + it.first_path * 8);
    }
}

hipError_t batch_path_errors_device(const DiagItem *d_items, const uint32_t *d_tile_item, uint32_t n_items, uint64_t n_tiles, uint64_t n_paths,
                                    uint32_t dims, uint64_t z, double ratio, uint64_t *d_head, uint64_t *d_tail, uint64_t *d_out,
                                    uint64_t max_blocks, hipStream_t st) {
    if (n_paths == 0 || n_items == 0) return hipSuccess;
    if (n_tiles)
        hipLaunchKernelGGL(batch_path_tiles_kernel, dim3(wave_grid(n_tiles, max_blocks)), dim3(Q_BLOCK), 0, st, d_items, d_tile_item, dims, z, ratio,
                           n_tiles, d_head, d_tail, d_out);
    hipLaunchKernelGGL(batch_path_combine_kernel, dim3(wave_grid(n_paths, max_blocks)), dim3(Q_BLOCK), 0, st, d_items, n_items, n_paths,
                       (const uint64_t *)d_head, (const uint64_t *)d_tail, d_out);
    return hipGetLastError();
}

// ---- K7i ------------------------------------------------------------------------------------------------------------------
// list == nullptr: counts[flat tile] = the tile's stretched pairs.  Otherwise offsets is the exclusive scan of the counts over
// ALL flat tiles: a tile's number inside its item is offsets[t] - offsets[first_tile], a difference of integers; the item's
// pair number k < min(cap, n_steps) goes to list[first_pair + k], in the item's own step and path numbering.  A tile whose
// first pair is already past the cap is skipped on the device: no count comes back to the host in between.
__global__ void __launch_bounds__(Q_BLOCK) batch_stretched_tiles_kernel(const DiagItem *__restrict__ items, const uint32_t *__restrict__ tile_item, const uint32_t dims,
                                                                        const uint64_t z, const double ratio, const uint64_t n_tiles,
                                                                        uint64_t *counts, const uint64_t *offsets, StretchedPair *list,
                                                                        const uint64_t cap) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t t = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; t < n_tiles; t += (uint64_t)gridDim.x * (Q_BLOCK / 64)) {
        const DiagItem it = items[wave_uniform(tile_item[t])];
        const uint64_t room = cap < it.n_steps ? cap : it.n_steps;
        uint64_t at = list ? offsets[t] - offsets[it.first_tile] : 0;       // number of the tile's next stretched pair in its item
        if (list && at >= room) continue;
        at = stretched_tile(it.step_rec, it.n_steps, it.x, it.n_nodes, dims, z, ratio, t - it.first_tile, lane, at,
                            list ? list + it.first_pair : nullptr, room);
        if (!list && lane == 0) counts[t] = at;
    }
}

// temporary storage of the one scan over n_tiles + 1 counts (a host-side question to rocPRIM: nothing is launched)
hipError_t batch_stretched_scan_bytes(uint64_t n_tiles, size_t *bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)(n_tiles + 1),
                                   rocprim::plus<uint64_t>(), (hipStream_t)nullptr);
}

// d_counts, d_offsets: n_tiles + 1 words each (offsets[first_tile[i + 1]] - offsets[first_tile[i]] is item i's total); d_list
// (nullable: count only): stretched_list_plan's entries; d_tmp: batch_stretched_scan_bytes.  Asynchronous on st.
hipError_t batch_stretched_pairs_device(const DiagItem *d_items, const uint32_t *d_tile_item, uint64_t n_tiles, uint32_t dims, uint64_t z,
                                        double ratio, uint64_t *d_counts, uint64_t *d_offsets, void *d_list, uint64_t cap, void *d_tmp,
                                        size_t tmp_bytes, uint64_t max_blocks, hipStream_t st) {
    if (n_tiles == 0) return hipSuccess;
    const unsigned blocks = wave_grid(n_tiles, max_blocks);
    hipError_t e = hipMemsetAsync(d_counts + n_tiles, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_stretched_tiles_kernel, dim3(blocks), dim3(Q_BLOCK), 0, st, d_items, d_tile_item, dims, z, ratio, n_tiles, d_counts,
                       (const uint64_t *)nullptr, (StretchedPair *)nullptr, (uint64_t)0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::exclusive_scan(d_tmp, tmp_bytes, d_counts, d_offsets, (uint64_t)0, (size_t)(n_tiles + 1), rocprim::plus<uint64_t>(), st);
    if (e != hipSuccess || !cap || !d_list) return e;
    hipLaunchKernelGGL(batch_stretched_tiles_kernel, dim3(blocks), dim3(Q_BLOCK), 0, st, d_items, d_tile_item, dims, z, ratio, n_tiles,
                       (uint64_t *)nullptr, (const uint64_t *)d_offsets, (StretchedPair *)d_list, cap);
    return hipGetLastError();
}

// ---- K7j ------------------------------------------------------------------------------------------------------------------
// slots: [item][pairs | stretched | max][n_nodes of the item], an item's at first_node * 3, zeroed by the caller.  Workgroup b
// is local block b - first_block of its item's own grid of `blocks` (K7g's plan): the pairs node_errors_kernel gives that
// block in the item's own launch — though sums of integers and a maximum would not mind another split.
__global__ void __launch_bounds__(Q_BLOCK) batch_node_errors_kernel(const DiagItem *items, const uint32_t *block_item, const uint32_t dims,
                                                                    const uint64_t z, const double ratio, unsigned long long *slots) {
    const DiagItem &it = items[block_item[blockIdx.x]];
    if (z >= it.n_steps) return;
    unsigned long long *pairs = slots + 3 * it.first_node, *stretched = pairs + it.n_nodes, *max_bits = pairs + 2 * it.n_nodes;
    const uint64_t n = it.n_steps - z, stride = (uint64_t)it.blocks * Q_BLOCK;
    for (uint64_t s = (uint64_t)(blockIdx.x - it.first_block) * Q_BLOCK + threadIdx.x; s < n; s += stride) {
        const uint4 ra = it.step_rec[s], rb = it.step_rec[s + z];
        double err, rel, dp, dl;
        bool st;
        if (!pair_stretch(ra, rb, it.x, it.n_nodes, dims, ratio, err, rel, dp, dl, st)) continue;
        node_pair(ra, rb, rel, st, pairs, stretched, max_bits);
    }
}
// out[first_node + k] = { pairs, stretched, max_rel_sq } of dense node k of its item (= gfs_node_error), through the item's layout
__global__ void batch_gather_node_errors_kernel(const DiagItem *items, const uint32_t n_items, const uint64_t n_nodes,
                                                const unsigned long long *slots, uint64_t *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += stride) {
        const DiagItem &it = items[diag_item_of(items, n_items, v, &DiagItem::first_node)];
        const unsigned long long *own = slots + 3 * it.first_node;
        const uint32_t slot = it.perm[v - it.first_node];
        out[3 * v] = own[slot]; out[3 * v + 1] = own[it.n_nodes + slot]; out[3 * v + 2] = own[2 * it.n_nodes + slot];
    }
}

// d_slots, d_out: 3 words per node of the union.  Asynchronous on st.
hipError_t batch_node_errors_device(const DiagItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks, uint64_t n_nodes,
                                    uint32_t dims, uint64_t z, double ratio, uint64_t *d_slots, uint64_t *d_out, hipStream_t st) {
    if (n_nodes == 0 || n_items == 0) return hipSuccess;
    if (row_blocks == 0 || row_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_slots, 0, 3 * n_nodes * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_node_errors_kernel, dim3((unsigned)row_blocks), dim3(Q_BLOCK), 0, st, d_items, d_block_item, dims, z, ratio,
                       reinterpret_cast<unsigned long long *>(d_slots));
    const uint64_t b = (n_nodes + 255) / 256;
    hipLaunchKernelGGL(batch_gather_node_errors_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(256), 0, st, d_items, n_items, n_nodes,
                       reinterpret_cast<const unsigned long long *>(d_slots), d_out);
    return hipGetLastError();
}

}  // namespace gfs
