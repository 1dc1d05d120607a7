// quality_kernels.hip — K7: how good are the positions that are in HBM now, read out on the device.
//   K7a  exhaustive pairs of path steps (s, s + z), for a list of step distances z: the relative error of
//        calculate_layout_stress (src/sgd.rs:1252-1275, Layout::distance) over ALL such pairs
//   K7b  the same per-pair value for a caller's list of step pairs (the device half of the sampled stress)
//   K7c  measure_layout_quality.rs:100-208 for the context's current 1D positions: rank order (K6), node lengths in rank
//        order, exclusive scan (rocPRIM), one pass over adjacent step pairs — all integers
//   K7d  K7a's figures per PATH for one step distance, with the path's step and reverse-step counts and its stretched pairs
//   K7e  the stretched pairs themselves, in ascending step order: count per tile, exclusive scan (rocPRIM), ordered write
//   K7f  per NODE: pairs and stretched pairs touching it, largest relative error (integer atomic adds, atomic max on bits)
// The kernels read step records and positions and write only their own output buffers.
//
// Determinism: the grid is a function of n_steps alone (quality_blocks), never of the device.  A thread accumulates its
// grid-stride pairs in order; the wave reduction is a fixed butterfly, the workgroup's is a sum in wave order; every
// workgroup stores its partials, and ONE thread per step distance sums them in workgroup order (reduce_partials_kernel).
// No floating-point atomics anywhere.
#include "sgd_host.h"
#include "device_memory.h"
#include "quality_device.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace gfs {

// Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS and the rule for a step pass's workgroups: batch_readout_plan.h.  The per-pair function
// (pair_error) and the fixed-tree reduction of a workgroup (combine, store_block_partials): quality_device.h, shared with K7g.
unsigned quality_blocks(uint64_t n_steps) { return quality_blocks_of(n_steps); }

// partials[field][zi][0..n_blocks) -> out[zi][field], summed in workgroup order by thread 0 (reduce_item_partials,
// quality_device.h).  One workgroup per step distance.
template <typename F>
__global__ void __launch_bounds__(Q_BLOCK) reduce_partials_kernel(const uint64_t *partials, const uint32_t n_blocks, uint64_t *out) {
    reduce_item_partials<F>(partials, gridDim.x, blockIdx.x, n_blocks, 0, n_blocks, out + (uint64_t)blockIdx.x * 5);
}

// ---- K7a ------------------------------------------------------------------------------------------------------------------
// grid (quality_blocks(n_steps), n_z).  Reads step_rec[0..n_steps) only: s + z < n_steps.
__global__ void __launch_bounds__(Q_BLOCK) pair_errors_kernel(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                              const uint32_t dims, const uint64_t *zs, uint64_t *partials) {
    const uint32_t zi = blockIdx.y;
    const uint64_t z = zs[zi];
    uint64_t pairs = 0;
    double sum_rel = 0.0, max_rel = 0.0, sum_abs = 0.0, sum_sq = 0.0;
    if (z < n_steps) {
        const uint64_t n = n_steps - z, stride = (uint64_t)gridDim.x * Q_BLOCK;
        for (uint64_t s = (uint64_t)blockIdx.x * Q_BLOCK + threadIdx.x; s < n; s += stride) {
            double err, rel;
            if (!pair_error(step_rec[s], step_rec[s + z], x, n_nodes, dims, err, rel)) continue;
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

// d_zs: n_z step distances; d_partials: 5 * n_z * quality_blocks(n_steps) words; d_out: n_z * 5 words
// { pairs (u64), sum_rel_sq, max_rel_sq, sum_abs, sum_sq (f64 bits) }.  Asynchronous on st.
hipError_t pair_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims,
                              const uint64_t *d_zs, uint32_t n_z, uint64_t *d_partials, uint64_t *d_out, hipStream_t st) {
    if (n_z == 0) return hipSuccess;
    const unsigned blocks = quality_blocks(n_steps);
    hipLaunchKernelGGL(pair_errors_kernel, dim3(blocks, n_z), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x, n_nodes, dims, d_zs, d_partials);
    hipLaunchKernelGGL(reduce_partials_kernel<PairFields>, dim3(n_z), dim3(Q_BLOCK), 0, st, d_partials, blocks, d_out);
    return hipGetLastError();
}

// ---- K7b ------------------------------------------------------------------------------------------------------------------
// rel_sq[i] of the pair (step_a[i], step_b[i]); -1 where the pair is skipped (also: a step beyond the table)
__global__ void __launch_bounds__(Q_BLOCK) pair_list_kernel(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                            const uint32_t dims, const uint64_t *step_a, const uint64_t *step_b, const uint64_t n,
                                                            double *rel_sq) {
    const uint64_t stride = (uint64_t)gridDim.x * Q_BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * Q_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint64_t sa = step_a[i], sb = step_b[i];
        double err, rel, out = -1.0;
        if (sa < n_steps && sb < n_steps && pair_error(step_rec[sa], step_rec[sb], x, n_nodes, dims, err, rel)) out = rel;
        rel_sq[i] = out;
    }
}
hipError_t pair_list_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims,
                            const uint64_t *d_step_a, const uint64_t *d_step_b, uint64_t n, double *d_rel_sq, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t b = (n + Q_BLOCK - 1) / Q_BLOCK;
    hipLaunchKernelGGL(pair_list_kernel, dim3((unsigned)(b > Q_MAX_BLOCKS ? Q_MAX_BLOCKS : b)), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x,
                       n_nodes, dims, d_step_a, d_step_b, n, d_rel_sq);
    return hipGetLastError();
}

// ---- K7c ------------------------------------------------------------------------------------------------------------------
// length of the node of rank r (0 for r = n_nodes, so that the scan's last element is the total)
struct RankLen {
    const uint32_t *order, *node_len;
    uint64_t n_nodes;
    __host__ __device__ uint64_t operator()(uint64_t r) const { return r >= n_nodes ? 0ull : (uint64_t)node_len[order[r]]; }
};
// sorted position of every node, by slot: spos[perm[order[r]]] = prefix[r]
__global__ void scatter_sorted_pos_kernel(const uint64_t *prefix, const uint32_t *order, const uint32_t *perm, uint64_t *spos, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) spos[perm[order[r]]] = prefix[r];
}
// adjacent steps of every path (sort_quality_pairs, quality_device.h).  Reads step_rec[0..n_steps) only.
__global__ void __launch_bounds__(Q_BLOCK) sort_quality_kernel(const uint4 *step_rec, const uint64_t n_steps, const uint64_t *spos, uint64_t *partials) {
    uint64_t steps = 0, abs_sum = 0, gen_sum = 0;
    double sq_sum = 0.0;
    sort_quality_pairs(step_rec, n_steps, spos, blockIdx.x, gridDim.x, steps, abs_sum, gen_sum, sq_sum);
    uint64_t v[5] = {steps, abs_sum, gen_sum, (uint64_t)__double_as_longlong(sq_sum), 0};
    store_block_partials<SortFields>(v, partials, 1, 0);
}

// The two halves of K7c, which a batch calls apart for its items above the sort cap (K7k, capi_batch.hip).
// First half.  d_order: rank -> dense index (sort_order_device).  d_prefix: n_nodes + 1 words; d_spos: n_nodes words, by slot.
// *total_len_out = the graph's length in bp; at 2^53 and beyond d_spos is not written (the caller refuses).  Synchronous up to
// the launch that writes d_spos.
hipError_t sorted_positions_device(const uint32_t *d_order, const uint32_t *d_node_len, const uint32_t *d_perm, uint64_t n_nodes,
                                   uint64_t *d_prefix, uint64_t *d_spos, uint64_t *total_len_out, hipStream_t st) {
    auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), RankLen{d_order, d_node_len, n_nodes});
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, lens, d_prefix, (uint64_t)0, (size_t)(n_nodes + 1), rocprim::plus<uint64_t>(), st);
    if (e != hipSuccess) return e;
    Buffer d_tmp;
    if ((e = d_tmp.grow(tmp_bytes ? tmp_bytes : 8)) != hipSuccess) return e;
    e = rocprim::exclusive_scan(d_tmp.p, tmp_bytes, lens, d_prefix, (uint64_t)0, (size_t)(n_nodes + 1), rocprim::plus<uint64_t>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(total_len_out, d_prefix + n_nodes, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    d_tmp.reset();                                                         // (here, before the launch below: not at the end of scope)
    if (e != hipSuccess || *total_len_out >= (1ull << 53)) return e;
    hipLaunchKernelGGL(scatter_sorted_pos_kernel, dim3(1024), dim3(256), 0, st, d_prefix, d_order, d_perm, d_spos, n_nodes);
    return hipGetLastError();
}
// Second half.  d_partials: 5 * quality_blocks(n_steps) words, d_out: 5 words { steps, abs_err_sum, genomic_sum (u64), sq_err_sum
// (f64 bits), 0 }.  Synchronous.
hipError_t sort_quality_steps_device(const uint4 *d_step_rec, uint64_t n_steps, const uint64_t *d_spos, uint64_t *d_partials, uint64_t *d_out,
                                     hipStream_t st) {
    const unsigned blocks = quality_blocks(n_steps);
    hipLaunchKernelGGL(sort_quality_kernel, dim3(blocks), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_spos, d_partials);
    hipLaunchKernelGGL(reduce_partials_kernel<SortFields>, dim3(1), dim3(Q_BLOCK), 0, st, d_partials, blocks, d_out);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}
// Both: at a length of 2^53 bp and beyond the pass is not run (the caller refuses).  Synchronous.
hipError_t sort_quality_device(const uint4 *d_step_rec, uint64_t n_steps, const uint32_t *d_order, const uint32_t *d_node_len,
                               const uint32_t *d_perm, uint64_t n_nodes, uint64_t *d_prefix, uint64_t *d_spos, uint64_t *d_partials,
                               uint64_t *d_out, uint64_t *total_len_out, hipStream_t st) {
    const hipError_t e = sorted_positions_device(d_order, d_node_len, d_perm, n_nodes, d_prefix, d_spos, total_len_out, st);
    if (e != hipSuccess || *total_len_out >= (1ull << 53)) return e;
    return sort_quality_steps_device(d_step_rec, n_steps, d_spos, d_partials, d_out, st);
}

// ---- K7d / K7e / K7f: which paths, pairs and nodes carry the error -----------------------------------------------------------
// The per-pair value is pair_error's; a counted pair is STRETCHED when d_layout / d_path > ratio, d_layout = err + d_path.
//
// Decomposition (K7d, K7e): the step table is cut into TILES of Q_TILE consecutive steps, a constant; one wave works a tile
// off in Q_TILE / 64 rounds of 64 consecutive steps, so what a tile yields does not depend on the grid that ran it.  A pair
// (s, s + z) belongs to the tile and to the path of s.  Q_TILE and the tile count: batch_readout_plan.h; what a wave does with
// a tile, a path or a pair (pair_stretch, path_tile, path_fold, stretched_tile, node_pair): quality_device.h, shared with K7h-j.
uint64_t quality_tiles(uint64_t n_steps) { return quality_tiles_of(n_steps); }
static unsigned tile_blocks(uint64_t n_steps) {
    const uint64_t b = (quality_tiles(n_steps) + Q_BLOCK / 64 - 1) / (Q_BLOCK / 64);
    return (unsigned)(b < 1 ? 1 : (b > Q_TILE_MAX_BLOCKS ? Q_TILE_MAX_BLOCKS : b));
}

// ---- K7d ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(Q_BLOCK) path_tiles_kernel(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                             const uint32_t dims, const uint64_t z, const double ratio, const uint64_t n_tiles,
                                                             uint64_t *head, uint64_t *tail, uint64_t *out) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t tile = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * (Q_BLOCK / 64))
        path_tile(step_rec, n_steps, x, n_nodes, dims, z, ratio, tile, lane, head, tail, out);
}

// One wave per path (path_fold).  path_rec: { first step lo, steps, -, first step hi }.
__global__ void __launch_bounds__(Q_BLOCK) path_combine_kernel(const uint4 *path_rec, const uint64_t n_paths, const uint64_t *head,
                                                               const uint64_t *tail, uint64_t *out) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t p = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; p < n_paths; p += (uint64_t)gridDim.x * (Q_BLOCK / 64))
        path_fold(path_rec[p], p, lane, head, tail, out);
}

// d_head, d_tail: 5 * quality_tiles(n_steps) words each; d_out: n_paths gfs_path_error (8 words each).  Asynchronous on st.
hipError_t path_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const uint4 *d_path_rec, uint64_t n_paths, const double *d_x,
                              uint64_t n_nodes, uint32_t dims, uint64_t z, double ratio, uint64_t *d_head, uint64_t *d_tail, uint64_t *d_out,
                              hipStream_t st) {
    if (n_paths == 0) return hipSuccess;
    const uint64_t tiles = quality_tiles(n_steps);
    if (tiles)
        hipLaunchKernelGGL(path_tiles_kernel, dim3(tile_blocks(n_steps)), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x, n_nodes, dims, z, ratio,
                           tiles, d_head, d_tail, d_out);
    const uint64_t b = (n_paths + Q_BLOCK / 64 - 1) / (Q_BLOCK / 64);
    hipLaunchKernelGGL(path_combine_kernel, dim3((unsigned)(b > Q_TILE_MAX_BLOCKS ? Q_TILE_MAX_BLOCKS : b)), dim3(Q_BLOCK), 0, st, d_path_rec,
                       n_paths, d_head, d_tail, d_out);
    return hipGetLastError();
}

// ---- K7e ------------------------------------------------------------------------------------------------------------------
// Two passes over the same tiles: the stretched pairs of every tile are counted (ballots), the counts scanned (rocPRIM),
// and the second pass writes pair number offset[tile] + (stretched pairs before it in the tile) where that is < cap: the
// list is in ascending step_a whatever ran when.  list == nullptr: the counting pass.
__global__ void __launch_bounds__(Q_BLOCK) stretched_tiles_kernel(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                                  const uint32_t dims, const uint64_t z, const double ratio, const uint64_t n_tiles,
                                                                  uint64_t *counts, const uint64_t *offsets, StretchedPair *list, const uint64_t cap) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t tile = (uint64_t)blockIdx.x * (Q_BLOCK / 64) + wave; tile < n_tiles; tile += (uint64_t)gridDim.x * (Q_BLOCK / 64)) {
        uint64_t at = list ? offsets[tile] : 0;                             // number of the tile's next stretched pair
        if (list && at >= cap) continue;
        at = stretched_tile(step_rec, n_steps, x, n_nodes, dims, z, ratio, tile, lane, at, list, cap);
        if (!list && lane == 0) counts[tile] = at;
    }
}

// d_counts, d_offsets: quality_tiles(n_steps) + 1 words each (the last offset is the total).  *total_out is on the host.
// d_list (nullable: count only): room for min(cap, n_steps) entries, of which min(cap, total) are written.  Synchronous.
hipError_t stretched_pairs_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims, uint64_t z,
                                  double ratio, uint64_t *d_counts, uint64_t *d_offsets, void *d_list, uint64_t cap, uint64_t *total_out,
                                  hipStream_t st) {
    *total_out = 0;
    const uint64_t tiles = quality_tiles(n_steps);
    if (tiles == 0) return hipSuccess;
    const unsigned blocks = tile_blocks(n_steps);
    hipError_t e = hipMemsetAsync(d_counts + tiles, 0, 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(stretched_tiles_kernel, dim3(blocks), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x, n_nodes, dims, z, ratio, tiles,
                       d_counts, (const uint64_t *)nullptr, (StretchedPair *)nullptr, (uint64_t)0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tmp_bytes = 0;
    e = rocprim::exclusive_scan(nullptr, tmp_bytes, d_counts, d_offsets, (uint64_t)0, (size_t)(tiles + 1), rocprim::plus<uint64_t>(), st);
    if (e != hipSuccess) return e;
    Buffer d_tmp;                                                          // (freed after the synchronise)
    if ((e = d_tmp.grow(tmp_bytes ? tmp_bytes : 8)) != hipSuccess) return e;
    e = rocprim::exclusive_scan(d_tmp.p, tmp_bytes, d_counts, d_offsets, (uint64_t)0, (size_t)(tiles + 1), rocprim::plus<uint64_t>(), st);
    if (e == hipSuccess) e = hipMemcpyAsync(total_out, d_offsets + tiles, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && cap && d_list) {
        hipLaunchKernelGGL(stretched_tiles_kernel, dim3(blocks), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x, n_nodes, dims, z, ratio, tiles,
                           (uint64_t *)nullptr, (const uint64_t *)d_offsets, (StretchedPair *)d_list, cap);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    return e != hipSuccess ? e : e2;
}

// ---- K7f ------------------------------------------------------------------------------------------------------------------
// Per node SLOT (node_pair, quality_device.h): integer atomic adds and an atomic max on bits.  slots: [pairs | stretched | max],
// n_nodes words each, zeroed by the caller.
__global__ void __launch_bounds__(Q_BLOCK) node_errors_kernel(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                              const uint32_t dims, const uint64_t z, const double ratio,
                                                              unsigned long long *slots) {
    if (z >= n_steps) return;
    unsigned long long *pairs = slots, *stretched = slots + n_nodes, *max_bits = slots + 2 * n_nodes;
    const uint64_t n = n_steps - z, stride = (uint64_t)gridDim.x * Q_BLOCK;
    for (uint64_t s = (uint64_t)blockIdx.x * Q_BLOCK + threadIdx.x; s < n; s += stride) {
        const uint4 ra = step_rec[s], rb = step_rec[s + z];
        double err, rel, dp, dl;
        bool st;
        if (!pair_stretch(ra, rb, x, n_nodes, dims, ratio, err, rel, dp, dl, st)) continue;
        node_pair(ra, rb, rel, st, pairs, stretched, max_bits);
    }
}
// out[k] = { pairs, stretched, max_rel_sq } of dense node k (= gfs_node_error)
__global__ void gather_node_errors_kernel(const unsigned long long *slots, const uint32_t *perm, const uint64_t n_nodes, uint64_t *out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_nodes; k += stride) {
        const uint32_t slot = perm[k];
        out[3 * k] = slots[slot]; out[3 * k + 1] = slots[n_nodes + slot]; out[3 * k + 2] = slots[2 * n_nodes + slot];
    }
}

// d_slots, d_out: 3 * n_nodes words each.  Asynchronous on st.
hipError_t node_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, const uint32_t *d_perm, uint64_t n_nodes,
                              uint32_t dims, uint64_t z, double ratio, uint64_t *d_slots, uint64_t *d_out, hipStream_t st) {
    if (n_nodes == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_slots, 0, 3 * n_nodes * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(node_errors_kernel, dim3(quality_blocks(n_steps)), dim3(Q_BLOCK), 0, st, d_step_rec, n_steps, d_x, n_nodes, dims, z, ratio,
                       reinterpret_cast<unsigned long long *>(d_slots));
    const uint64_t b = (n_nodes + 255) / 256;
    hipLaunchKernelGGL(gather_node_errors_kernel, dim3((unsigned)(b > 1024 ? 1024 : b)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned long long *>(d_slots), d_perm, n_nodes, d_out);
    return hipGetLastError();
}

hipError_t warm_module_quality() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&pair_errors_kernel));
}

}  // namespace gfs
