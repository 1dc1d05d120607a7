// index_set.h — what capi_set.hip and index_set_kernels.hip share: the index build of MANY graphs in one pass (K3b).  The items are
// treated as one disjoint graph — their nodes, steps and paths concatenated (the UNION) — and an item table says where each item
// begins in the union and where its five index arrays lie in the set's arena.  Nothing here is exported from the shared object.
#pragma once
#include "index_set_plan.h"
#include "launch_policy.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// Item i of a set; the table holds one more entry, whose three union offsets are the totals (its arena offsets are unused).
struct SetItem {
    uint64_t node_off, step_off, path_off;       // first union node / step / path of the item
    uint64_t rec, prec, plen, perm, nlen;        // byte offsets into the arena: step records (n_steps + 1), path records, path
};                                               // lengths, node layout, node lengths (gfs_ctx_set_plan)
static_assert(sizeof(SetItem) == SET_ITEM_BYTES, "the item table of the input head (index_set_plan.h)");

// The union as the kernels see it; every pointer is a device pointer.  step_node keeps each item's OWN dense indices (a kernel
// adds the item's node_off); path_first is in union steps, [n_paths + 1], its last entry n_steps.
struct SetUnion {
    uint32_t n_items;
    uint64_t n_nodes, n_steps, n_paths;
    const SetItem *items;                        // [n_items + 1]
    const uint32_t *step_node;                   // [n_steps]
    const uint8_t *step_is_rev;                  // [n_steps]
    const uint64_t *path_first;                  // [n_paths + 1]
    unsigned char *arena;                        // zeroed; every item's node lengths already in place
    uint2 *trip;                                 // a union of ONE item: its 8-byte trip records, [n_steps + 1]; else null
};

constexpr uint32_t SET_NO_BAD_ITEM = 0xFFFFFFFFu;
constexpr unsigned SET_STEP_BLOCKS = 2048, SET_NODE_BLOCKS = 1024, SET_PATH_BLOCKS = 64, SET_BLOCK = 256;   // the grids of the kernels over steps / over nodes / over paths and items

// Bytes of scratch the build needs for a union of these totals (rocPRIM's temporary storage included).
hipError_t index_set_work_bytes(uint64_t n_nodes, uint64_t n_steps, uint64_t *bytes);
// The build, in its two halves; both on the null stream, over the same d_work.  *launches += kernel launches and memsets, each
// rocPRIM call counted as one.
// Layout half: the range check of step_node — *bad_item = lowest item with a step naming a node out of its range (nothing that
// indexes by step_node has run then), else SET_NO_BAD_ITEM — and then every item's node layout into its perm range of the arena.
// layout_given: the perm ranges already hold the caller's layout; only the range check runs.
hipError_t index_set_layout_device(const SetUnion &u, void *d_work, bool layout_given, uint32_t *bad_item, uint64_t *launches);
// K3 half, after the layouts are in place: every item's step records (padding record included), path records and path lengths.
// The arena is complete once the stream has drained.  Where u.trip is set the pass that writes the step records writes
// trip[s] = { slot, pos lo } beside them.  facts (nullable): the largest position and crowding exponents of the records, reduced in
// that same pass and read back with one blocking copy (have_trip_rec is left to the caller).
hipError_t index_set_records_device(const SetUnion &u, void *d_work, uint64_t *launches, RecordFacts *facts = nullptr);
hipError_t warm_module_index_set();

}  // namespace gfs
