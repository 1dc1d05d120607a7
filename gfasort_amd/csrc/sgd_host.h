// sgd_host.h — the host-side interface between the translation units of libgfasort_hip.so: the only declaration of
// everything one unit calls in another.  The kernel units SELECT (shape -> address of the kernel, null where no such kernel is
// built); capi.hip resolves a context's kernels once, when the context is set up, and launches them through one path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "capi_error.h"                                   // gfs_set_error
#include "sgd_limits.h"                                   // pool_bytes, nd_team_waves

namespace gfs {

// What picks a kernel: dims 0 = the 1D sort, 1..8 = layouts; bundle 0 / 1 = reference streams, 4..64 = team kernels.
// compact: the build of K1b / K1c at B = 64 whose trips read 8-byte trip records (sgd_1d.h TripRec); no other kernel has one.
struct KernelShape { int dims; uint32_t bundle; bool lds_tables, atomic_loads, trace; bool compact = false; };

template <typename... A> inline const void *kernel_addr(void (*k)(A...)) { return reinterpret_cast<const void *>(k); }
// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F> inline auto with_flag(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// One iteration per launch, kernel(KArgs).  K1 / K2 (reference streams) are built for every combination of the three flags.
// The team kernels' trace variants always read with agent-scope loads, and the layout team kernels (K2b) have no other loads:
// they ignore atomic_loads.  K1b exists for B = 4..64, K2b for B = 8..64: D = 1..3 in one unit, D = 4..8 in another, so that
// the two compile side by side.
const void *iteration_kernel_1d(const KernelShape &s);              // sgd_kernels_1d.hip: K1, K1b
const void *iteration_kernel_nd(const KernelShape &s);              // sgd_kernels_nd.hip: K2
const void *iteration_kernel_nd_team(const KernelShape &s);         // sgd_kernels_nd_team.hip: K2b, D = 1..3
const void *iteration_kernel_nd_team_wide(const KernelShape &s);    // sgd_kernels_nd_team_wide.hip: K2b, D = 4..8

// A range of iterations per launch, kernel(KArgs, const IterConsts *, uint32_t n_iters, uint32_t *pool).  pooled: the waves
// draw an iteration's updates from pool (zeroed counters, pool_bytes(n_iters) of them); otherwise fixed quotas per wave,
// free-running, and pool is null.  The fused kernels are built with agent-scope loads and without trace only — a context
// with other flags does not fuse — so those two fields are not looked at.  Reference streams (K1d, K2d) and the phased
// sampler (K1e) have no free-running form; K1c exists for B = 16, 32, 64, K2c for B = 64 and D = 2..8.
const void *fused_kernel_1d(const KernelShape &s, bool pooled);             // sgd_kernels_1d.hip: K1d, K1c
const void *phased_fused_kernel(bool lds_tables);                           // sgd_kernels_1d_phased.hip: K1e
const void *fused_kernel_nd(const KernelShape &s, bool pooled);             // sgd_kernels_nd.hip: K2d
const void *fused_kernel_nd_team(const KernelShape &s, bool pooled);        // sgd_kernels_nd_team.hip: K2c, D = 2, 3
const void *fused_kernel_nd_team_wide(const KernelShape &s, bool pooled);   // sgd_kernels_nd_team_wide.hip: K2c, D = 4..8

// Many contexts per launch, kernel(const BatchItem *items, const uint32_t *block_item) (sgd_batch.h): K1d's body (dims 0) or K2d's
// (dims 2, 3) on the item that block_item[blockIdx.x] names.  Null for other dimensions.
const void *batch_fused_kernel(int dims, bool lds_tables);                  // sgd_kernels_batch.hip: K1f, K2f

// HIP loads a translation unit's code object on first use: each of these touches one kernel of its unit (gfs_warmup)
hipError_t warm_module_1d();
hipError_t warm_module_1d_phased();
hipError_t warm_module_nd();
hipError_t warm_module_nd_team();
hipError_t warm_module_nd_team_wide();
hipError_t warm_module_index();
hipError_t warm_module_quality();

// index_kernels.hip
hipError_t init_positions_device(const uint32_t *d_node_len, const uint32_t *d_perm, double *d_x, uint64_t n);
hipError_t reorder_positions_device(const double *d_src, double *d_dst, const uint32_t *d_perm, uint64_t N, uint32_t D,
                                    int to_device, hipStream_t st);
hipError_t sort_order_device(const double *d_x_layout, const uint32_t *d_perm, uint64_t n, uint64_t stride_doubles,
                             void *d_tmp, uint32_t **d_order_out);
// what d_tmp must hold for n nodes: two buffers of keys and two of values
inline uint64_t sort_order_scratch_bytes(uint64_t n) { return n * (2 * 8 + 2 * 4); }

// batch_readout_kernels.hip (K4b, K6b): one workgroup per item of a table on the device.  x, perm and node_len are the item's
// context's; offset is where its segment starts in the packed outputs; padded = segment_padded(n) (segment_sort.h; K6b only).
struct ReadoutItem {
    double *x;
    const uint32_t *perm, *node_len;
    uint64_t offset;
    uint32_t n, padded;
};
static_assert(sizeof(ReadoutItem) == 40, "a multiple of 8 bytes: the next part of a read-out's region starts where the table ends (readout_region.h)");
// K4b: every item's initial positions (what init_positions_device writes).  Asynchronous.
hipError_t batch_init_positions_device(const ReadoutItem *d_items, uint32_t count, hipStream_t st);
// K6b: count items of one padded length <= SEGMENT_SORT_CAP: d_positions (nullable) [offset + k] = x[perm[k]], d_order[offset + r] =
// dense index of the node of rank r.  Asynchronous.
hipError_t sort_segments_device(const ReadoutItem *d_items, uint32_t count, uint32_t padded, double *d_positions, uint32_t *d_order,
                                hipStream_t st);

// batch_quality_kernels.hip (K4c / K6c, K7g): flat launches over all items of a batch; workgroup b works on item block_item[b] and
// is that item's local block b - first_block (batch_readout_plan.h builds first_block and block_item).
// K4c / K6c: x, perm and n are the item's context's (dims = D >= 1: x is the end x dimension planes); offset is the item's first
// word in the packed array, Layout.coords order.  first_block counts workgroups of COORD_BLOCK words.
struct CoordItem {
    double *x;
    const uint32_t *perm;
    uint64_t offset;
    uint32_t n, first_block, dims, _pad;
};
static_assert(sizeof(CoordItem) == 40, "a multiple of 8 bytes: the next part of a read-out's region starts where the table ends (readout_region.h)");
// to_device = 1: packed -> the items' planes (what reorder_positions_device writes per item), else planes -> packed.  Asynchronous.
hipError_t batch_coords_device(const CoordItem *d_items, const uint32_t *d_block_item, uint64_t blocks, double *d_packed, int to_device,
                               hipStream_t st);
// K7g: blocks = quality_blocks(n_steps), first_block = the sum of the blocks of the items before it.
struct QualityItem {
    const uint4 *step_rec;
    const double *x;
    uint64_t n_steps, n_nodes;
    uint32_t first_block, blocks;
};
static_assert(sizeof(QualityItem) == 40, "a multiple of 8 bytes: the next part of a read-out's region starts where the table ends (readout_region.h)");
// All pairs (s, s + z) of every item for n_z step distances.  row_blocks: the sum of the items' blocks; d_partials: 5 * n_z *
// row_blocks words; d_out: 5 words per (item, distance), [item][z], as pair_errors_device writes them for one.  Asynchronous.
hipError_t batch_pair_errors_device(const QualityItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks,
                                    uint32_t dims, const uint64_t *d_zs, uint32_t n_z, uint64_t *d_partials, uint64_t *d_out, hipStream_t st);

// batch_diagnosis_kernels.hip (K7h, K7i, K7j): K7d / K7e / K7f of every item of a batch, for one step distance z and one ratio.
// step_rec, path_rec, x and perm are the item's context's.  first_tile, first_path, first_node, first_pair: where the item's
// tiles (tile_plan), paths and nodes (row_offsets) and its room in the packed list of stretched pairs (stretched_list_plan) start;
// first_block, blocks: K7g's plan (quality_plan).  All of it from batch_readout_plan.h.
struct DiagItem {
    const uint4 *step_rec, *path_rec;
    const double *x;
    const uint32_t *perm;
    uint64_t n_steps, n_nodes, n_paths;
    uint64_t first_tile, first_path, first_node, first_pair;
    uint32_t first_block, blocks;
};
static_assert(sizeof(DiagItem) == 96, "a multiple of 8 bytes: the next part of a read-out's region starts where the table ends (readout_region.h)");
// max_blocks (K7h, K7i): a cap on the grids over flat tiles and paths below Q_TILE_MAX_BLOCKS, 0 = none (a test hook: a tile's
// yield does not depend on the grid).
// K7h: d_tile_item: n_tiles entries; d_head, d_tail: 5 words per flat tile; d_out: 8 words per path of the union, item i's rows at
// first_path, as path_errors_device writes them for one.  Two launches.  Asynchronous.
hipError_t batch_path_errors_device(const DiagItem *d_items, const uint32_t *d_tile_item, uint32_t n_items, uint64_t n_tiles, uint64_t n_paths,
                                    uint32_t dims, uint64_t z, double ratio, uint64_t *d_head, uint64_t *d_tail, uint64_t *d_out,
                                    uint64_t max_blocks, hipStream_t st);
// K7i: d_counts, d_offsets: n_tiles + 1 words each; item i's total is d_offsets[first_tile[i + 1]] - d_offsets[first_tile[i]];
// d_list (nullable: count only): the first min(cap, total) pairs of item i at first_pair, in ascending step_a, the entries
// stretched_pairs_device writes for one; d_tmp, tmp_bytes: batch_stretched_scan_bytes(n_tiles).  Two launches, a memset, one scan.
// Asynchronous: the cap is tested on the device.
hipError_t batch_stretched_scan_bytes(uint64_t n_tiles, size_t *bytes);
hipError_t batch_stretched_pairs_device(const DiagItem *d_items, const uint32_t *d_tile_item, uint64_t n_tiles, uint32_t dims, uint64_t z,
                                        double ratio, uint64_t *d_counts, uint64_t *d_offsets, void *d_list, uint64_t cap, void *d_tmp,
                                        size_t tmp_bytes, uint64_t max_blocks, hipStream_t st);
// K7j: d_block_item: row_blocks entries; d_slots, d_out: 3 words per node of the union; d_out by dense index, item i's rows at
// first_node, as node_errors_device writes them for one.  Two launches and a memset.  Asynchronous.
hipError_t batch_node_errors_device(const DiagItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks, uint64_t n_nodes,
                                    uint32_t dims, uint64_t z, double ratio, uint64_t *d_slots, uint64_t *d_out, hipStream_t st);

// batch_sort_quality_kernels.hip (K7k): K7c of every item of a batch of 1D sorts.
// a: count items of one padded length <= SEGMENT_SORT_CAP, one workgroup each (ReadoutItem as for K6b; offset = the item's first
// node in d_spos): d_spos[offset + slot] = the sorted position of the node in that slot, as sorted_positions_device writes it for
// one; d_totals[row] = the item's length in bp.  Asynchronous.
hipError_t batch_sorted_positions_device(const ReadoutItem *d_items, uint32_t count, uint32_t padded, uint64_t *d_spos, uint64_t *d_totals,
                                         hipStream_t st);
// b, c: spos = the item's part of d_spos; first_block, blocks: K7g's plan (quality_plan).
struct SortQualityItem {
    const uint4 *step_rec;
    const uint64_t *spos;
    uint64_t n_steps;
    uint32_t first_block, blocks;
};
static_assert(sizeof(SortQualityItem) == 32, "a multiple of 8 bytes: the next part of a read-out's region starts where the table ends (readout_region.h)");
// d_block_item: row_blocks entries; d_partials: 5 * row_blocks words; d_out: 5 words per item, as sort_quality_steps_device writes
// them for one.  Two launches.  Asynchronous.
hipError_t batch_sort_quality_device(const SortQualityItem *d_items, const uint32_t *d_block_item, uint32_t n_items, uint64_t row_blocks,
                                     uint64_t *d_partials, uint64_t *d_out, hipStream_t st);

// quality_kernels.hip (K7): read-outs of the resident positions.  They write their own output buffers only.
// Workgroups of the step passes: a function of n_steps alone, so that a result does not depend on the device.
unsigned quality_blocks(uint64_t n_steps);
// K7a: all pairs of steps (s, s + z) for n_z step distances.  d_partials: 5 * n_z * quality_blocks(n_steps) words;
// d_out: 5 words per distance { pairs (u64), sum_rel_sq, max_rel_sq, sum_abs, sum_sq (f64 bits) }.  Asynchronous.
hipError_t pair_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims,
                              const uint64_t *d_zs, uint32_t n_z, uint64_t *d_partials, uint64_t *d_out, hipStream_t st);
// K7b: d_rel_sq[i] of the pair (d_step_a[i], d_step_b[i]), -1 where it is skipped.  Asynchronous.
hipError_t pair_list_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims,
                            const uint64_t *d_step_a, const uint64_t *d_step_b, uint64_t n, double *d_rel_sq, hipStream_t st);
// K7c: d_order from sort_order_device; d_prefix: n_nodes + 1 words, d_spos: n_nodes, d_partials: 5 * quality_blocks(n_steps),
// d_out: 5 words { steps, abs_err_sum, genomic_sum (u64), sq_err_sum (f64 bits), 0 }; not run where *total_len_out >= 2^53.
// Synchronous.  Its two halves, which K7k calls apart for items above the sort cap: the sorted position of every node by slot
// (d_spos is not written where *total_len_out >= 2^53), and the step pass with its reduce.
hipError_t sorted_positions_device(const uint32_t *d_order, const uint32_t *d_node_len, const uint32_t *d_perm, uint64_t n_nodes,
                                   uint64_t *d_prefix, uint64_t *d_spos, uint64_t *total_len_out, hipStream_t st);
hipError_t sort_quality_steps_device(const uint4 *d_step_rec, uint64_t n_steps, const uint64_t *d_spos, uint64_t *d_partials, uint64_t *d_out,
                                     hipStream_t st);
hipError_t sort_quality_device(const uint4 *d_step_rec, uint64_t n_steps, const uint32_t *d_order, const uint32_t *d_node_len,
                               const uint32_t *d_perm, uint64_t n_nodes, uint64_t *d_prefix, uint64_t *d_spos, uint64_t *d_partials,
                               uint64_t *d_out, uint64_t *total_len_out, hipStream_t st);
// K7d / K7e / K7f, for one step distance z; a counted pair is stretched when (err + d_path) / d_path > ratio.  K7d and K7e cut the
// step table into tiles of a constant number of steps: quality_tiles(n_steps) of them.
uint64_t quality_tiles(uint64_t n_steps);
// K7d: d_path_rec as the SGD kernels read it; d_head, d_tail: 5 * quality_tiles(n_steps) words each; d_out: 8 words per path
// { steps, reverse_steps, pairs (u64), sum_rel_sq, max_rel_sq, sum_abs, sum_sq (f64 bits), stretched (u64) }.  Asynchronous.
hipError_t path_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const uint4 *d_path_rec, uint64_t n_paths, const double *d_x,
                              uint64_t n_nodes, uint32_t dims, uint64_t z, double ratio, uint64_t *d_head, uint64_t *d_tail, uint64_t *d_out,
                              hipStream_t st);
// K7e: d_counts, d_offsets: quality_tiles(n_steps) + 1 words each; d_list (nullable: count only): room for min(cap, n_steps)
// entries { step_a, step_b, path (u64), d_path, d_layout (f64) }, of which the first min(cap, *total_out) are written, in
// ascending step_a.  Synchronous.
hipError_t stretched_pairs_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, uint64_t n_nodes, uint32_t dims, uint64_t z,
                                  double ratio, uint64_t *d_counts, uint64_t *d_offsets, void *d_list, uint64_t cap, uint64_t *total_out,
                                  hipStream_t st);
// K7f: d_slots, d_out: 3 * n_nodes words each; d_out by dense index { pairs, stretched (u64), max_rel_sq (f64 bits) }.  Asynchronous.
hipError_t node_errors_device(const uint4 *d_step_rec, uint64_t n_steps, const double *d_x, const uint32_t *d_perm, uint64_t n_nodes,
                              uint32_t dims, uint64_t z, double ratio, uint64_t *d_slots, uint64_t *d_out, hipStream_t st);

// sgd_kernels_1d.hip: the multi-GPU replica merge
hipError_t launch_merge_prepare(const double *x, const double *x_prev, float *buf, uint64_t n, hipStream_t st);
hipError_t launch_merge_apply(double *x, double *x_prev, const float *buf, uint64_t n, double scale_all, hipStream_t st);

}  // namespace gfs
