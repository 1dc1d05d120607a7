// index_set.h — what capi_set.hip and index_set_kernels.hip share: the index build of MANY graphs in one pass (K3b).  The items are
// treated as one disjoint graph — their nodes, steps and paths concatenated (the UNION) — and an item table says where each item
// begins in the union and where its five index arrays lie in the set's arena.  Nothing here is exported from the shared object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

// Item i of a set; the table holds one more entry, whose three union offsets are the totals (its arena offsets are unused).
struct SetItem {
    uint64_t node_off, step_off, path_off;       // first union node / step / path of the item
    uint64_t rec, prec, plen, perm, nlen;        // byte offsets into the arena: step records (n_steps + 1), path records, path
};                                               // lengths, node layout, node lengths (gfs_ctx_set_plan)

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
};

constexpr uint32_t SET_NO_BAD_ITEM = 0xFFFFFFFFu;
constexpr unsigned SET_STEP_BLOCKS = 2048, SET_NODE_BLOCKS = 1024, SET_PATH_BLOCKS = 64, SET_BLOCK = 256;   // the grids of the kernels over steps / over nodes / over paths and items

// Bytes of scratch build_index_set_device needs for a union of these totals (rocPRIM's temporary storage included).
hipError_t index_set_work_bytes(uint64_t n_nodes, uint64_t n_steps, uint64_t *bytes);
// Fills every item's step records (padding record included), path records, path lengths and node layout in the arena.
// *bad_item = lowest item with a step naming a node out of its range (nothing past the range check has run then), else
// SET_NO_BAD_ITEM.  *launches += kernel launches and memsets, each rocPRIM call counted as one.  On the null stream; the arena is
// complete once the stream has drained (the last call in here is a blocking copy only where a fixpoint ran).
hipError_t build_index_set_device(const SetUnion &u, void *d_work, uint32_t *bad_item, uint64_t *launches);
hipError_t warm_module_index_set();

}  // namespace gfs
