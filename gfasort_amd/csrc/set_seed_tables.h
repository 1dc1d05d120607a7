// set_seed_tables.h — the seeding kernel's tables behind the state arrays of a setup's arena (capi_set.hip setup_contexts), host
// arithmetic only: where they lie and what goes into them.  Plain C++, so that a test compiles it alone; Item is set_seed.h's
// SeedItem { rng, first, n_streams, first_block } or a mirror of it.
#pragma once
#include "index_set_plan.h"                        // round256

#include <stdint.h>
#include <string.h>

namespace gfs {

// [items | block table] of the launch over all items with streams, then, for gfs_ctx_reset_streams, [every item once more as the
// only one of a launch: first_block 0 | that launch's block table: zeros, as long as the widest item's]
struct SeedTables { uint64_t items_at, blocks_at, alone_at, zeros_at, end; };
inline SeedTables seed_tables_plan(uint64_t begin, uint64_t n_items, uint64_t item_bytes, uint64_t total_blocks, uint64_t most_blocks) {
    SeedTables t;
    t.items_at = begin; t.blocks_at = t.items_at + round256(n_items * item_bytes);
    t.alone_at = t.blocks_at + round256(total_blocks * sizeof(uint32_t)); t.zeros_at = t.alone_at + round256(n_items * item_bytes);
    t.end = t.zeros_at + round256(most_blocks * sizeof(uint32_t));
    return t;
}
// into a zeroed mirror of [begin, end): `base` is where offset `begin` lies.  block_size: streams per workgroup.
template <class Item> inline void fill_seed_tables(const SeedTables &t, const Item *items, uint64_t n_items, uint32_t block_size, unsigned char *base) {
    uint32_t *block_item = reinterpret_cast<uint32_t *>(base + (t.blocks_at - t.items_at));
    for (uint64_t k = 0; k < n_items; ++k) {
        const uint64_t nb = ((uint64_t)items[k].n_streams + block_size - 1) / block_size;
        for (uint64_t b = 0; b < nb; ++b) block_item[items[k].first_block + b] = (uint32_t)k;
        Item alone = items[k];
        alone.first_block = 0;
        memcpy(base + k * sizeof(Item), &items[k], sizeof(Item));
        memcpy(base + (t.alone_at - t.items_at) + k * sizeof(Item), &alone, sizeof(Item));
    }
}

}  // namespace gfs
