// batch_readout_plan.h — which workgroup, or which wave, of a batch's flat read-out launches works on which item (K4c / K6c, K7g:
// batch_quality_kernels.hip; K7h / K7i / K7j: batch_diagnosis_kernels.hip; K7k: batch_sort_quality_kernels.hip), where an item's
// rows lie in the packed results, and in which order the one-workgroup-per-item launches (K6b, K7k) take the items.
// Host only and free of HIP: the kernels take every index from the tables built here, and tests/test_batch_layout_host.py,
// tests/test_batch_diagnosis_host.py and tests/test_batch_sort_quality_host.py compile it into programs of their own under the
// address and undefined-behaviour sanitizers.
#pragma once
#include "segment_sort.h"                                 // segment_padded, SEGMENT_SORT_CAP (free of HIP as well)
#include <stdint.h>

namespace gfs {

// ---- K7: workgroups of a step pass ----------------------------------------------------------------
// A function of n_steps alone, never of the device (quality_kernels.hip: what makes a figure reproducible).
constexpr unsigned Q_BLOCK = 256, Q_PAIRS_PER_THREAD = 8, Q_MAX_BLOCKS = 2048;
inline unsigned quality_blocks_of(uint64_t n_steps) {
    const uint64_t per_block = (uint64_t)Q_BLOCK * Q_PAIRS_PER_THREAD;
    const uint64_t b = n_steps / per_block + (n_steps % per_block != 0);
    return (unsigned)(b < 1 ? 1 : (b > Q_MAX_BLOCKS ? Q_MAX_BLOCKS : b));
}

// ---- K7g: item i owns quality_blocks_of(n_steps[i]) consecutive workgroups of every step distance's grid row ----------
// first_block[0..n]: prefix sums (first_block[n] = the row's length).  Inside, workgroup b of item i is local block
// b - first_block[i] of a grid of first_block[i + 1] - first_block[i]: the pair (block, grid) the item's own launch has.
inline uint64_t quality_plan(const uint64_t *n_steps, uint64_t n, uint64_t *first_block) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) { first_block[i] = total; total += quality_blocks_of(n_steps[i]); }
    first_block[n] = total;
    return total;
}

// ---- K4c / K6c: item i has n_nodes[i] * 2 * D words of coordinates, packed in item order -------------------------------
// A workgroup moves COORD_BLOCK consecutive words of ONE item: item i owns coord_blocks(words of i) consecutive workgroups
// (none where it has no node), so that a workgroup reads its item once and the packed side is walked in order.
constexpr unsigned COORD_BLOCK = 256;
inline uint64_t coord_blocks(uint64_t words) { return words / COORD_BLOCK + (words % COORD_BLOCK != 0); }
// word_offset[0..n], first_block[0..n]: prefix sums; returns the launch's workgroups (first_block[n]).
inline uint64_t coord_plan(const uint64_t *n_nodes, uint64_t n, uint32_t D, uint64_t *word_offset, uint64_t *first_block) {
    uint64_t words = 0, blocks = 0;
    for (uint64_t i = 0; i < n; ++i) {
        word_offset[i] = words; first_block[i] = blocks;
        const uint64_t w = n_nodes[i] * 2 * (uint64_t)D;
        words += w; blocks += coord_blocks(w);
    }
    word_offset[n] = words; first_block[n] = blocks;
    return blocks;
}

// block -> item for either plan: block_item[b] = i for first_block[i] <= b < first_block[i + 1]; block_item has
// first_block[n] entries.  (Read per workgroup as K1f reads its block table: no search on the device.)
inline void block_item_table(const uint64_t *first_block, uint64_t n, uint32_t *block_item) {
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t b = first_block[i]; b < first_block[i + 1]; ++b) block_item[b] = (uint32_t)i;
}

// ---- K7d / K7e and their batch forms K7h / K7i: tiles of Q_TILE consecutive steps, one wave each -----------------------
// A constant: what a tile yields does not depend on the grid that ran it (quality_kernels.hip).
constexpr unsigned Q_TILE = 512, Q_TILE_ROUNDS = Q_TILE / 64, Q_TILE_MAX_BLOCKS = 16384;
inline uint64_t quality_tiles_of(uint64_t n_steps) { return n_steps / Q_TILE + (n_steps % Q_TILE != 0); }

// Item i owns quality_tiles_of(n_steps[i]) consecutive tiles of one flat tile space, none where it has no step.
// first_tile[0..n]: prefix sums; returns the flat tiles (first_tile[n]).  Flat tile t of item i is the item's LOCAL tile
// t - first_tile[i]: steps [local * Q_TILE, min(local * Q_TILE + Q_TILE, n_steps[i])) of the item's own table.
inline uint64_t tile_plan(const uint64_t *n_steps, uint64_t n, uint64_t *first_tile) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) { first_tile[i] = total; total += quality_tiles_of(n_steps[i]); }
    first_tile[n] = total;
    return total;
}
// tile -> item: tile_item[t] = i for first_tile[i] <= t < first_tile[i + 1]; first_tile[n] entries (read per wave, never searched)
inline void tile_item_table(const uint64_t *first_tile, uint64_t n, uint32_t *tile_item) { block_item_table(first_tile, n, tile_item); }

// Where item i's rows start in a packed per-path or per-node output: first[0..n], prefix sums of count[0..n); returns the
// total.  (Over the items' nodes these are gfs_batch_result_offsets; over their paths, gfs_batch_path_offsets.)
inline uint64_t row_offsets(const uint64_t *count, uint64_t n, uint64_t *first) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) { first[i] = total; total += count[i]; }
    first[n] = total;
    return total;
}

// K7i's packed list of stretched pairs on the device: item i has room for min(cap, n_steps[i]) entries (it has fewer pairs
// than steps), at first_pair[i]; first_pair[0..n]; returns the entries of all items.
inline uint64_t stretched_room(uint64_t cap, uint64_t n_steps) { return cap < n_steps ? cap : n_steps; }
inline uint64_t stretched_list_plan(const uint64_t *n_steps, uint64_t n, uint64_t cap, uint64_t *first_pair) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) { first_pair[i] = total; total += stretched_room(cap, n_steps[i]); }
    first_pair[n] = total;
    return total;
}

// ---- K6b / K7k: one launch per padded segment length -------------------------------------------------------------------
// An item of at most `cap` nodes (cap <= SEGMENT_SORT_CAP) is sorted in LDS by one workgroup, in a launch with the other items of
// its padded length (the launch's LDS and block are sized by it); one of more nodes takes K6, alone.
constexpr uint64_t SEGMENT_ABOVE_CAP = ~0ull;
inline uint64_t segment_group_of(uint64_t n_nodes, uint64_t cap) { return n_nodes <= cap ? (uint64_t)segment_padded((uint32_t)n_nodes) : SEGMENT_ABOVE_CAP; }
// order[0..n): the items by ascending padded length, those above the cap last, item order kept among equals (what a stable sort
// by segment_group_of gives).  Returns how many are within the cap: order[0 .. that) are the launches' rows.
inline uint64_t segment_launch_order(const uint64_t *n_nodes, uint64_t n, uint64_t cap, uint64_t *order) {
    uint64_t at = 0, within = 0;
    for (uint64_t P = SEGMENT_WAVE;; P <<= 1) {
        const uint64_t group = P <= SEGMENT_SORT_CAP ? P : SEGMENT_ABOVE_CAP;
        if (group == SEGMENT_ABOVE_CAP) within = at;
        for (uint64_t i = 0; i < n; ++i) if (segment_group_of(n_nodes[i], cap) == group) order[at++] = i;
        if (group == SEGMENT_ABOVE_CAP) break;
    }
    return within;
}
// the row behind the last one of the launch that starts at row `first` (< within): the rows of one padded length
// (kept out of line, as it has been: called once per launch, and the shared object's list of symbols stays what it was)
__attribute__((noinline)) inline uint64_t segment_launch_end(const uint64_t *n_nodes, const uint64_t *order, uint64_t first, uint64_t within, uint64_t cap) {
    const uint64_t P = segment_group_of(n_nodes[order[first]], cap);
    uint64_t end = first;
    while (end < within && segment_group_of(n_nodes[order[end]], cap) == P) ++end;
    return end;
}

}  // namespace gfs
