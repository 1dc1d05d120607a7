// set_seed.h — what capi_set.hip and set_setup_kernels.hip share: the two tables of the launch that seeds every RNG stream of every
// item of a context set (K3c).  Nothing here is exported from the shared object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

constexpr uint32_t SEED_BLOCK = 256;             // threads per workgroup; an item takes ceil(n_streams / SEED_BLOCK) workgroups of its own

// One item with streams, for the seeding kernel.
struct SeedItem {
    uint64_t *rng;                               // the item's [4][n_streams] words, on the device
    uint64_t first;                              // seed + stream_base, wrapping: stream t is seeded from first + t
    uint32_t n_streams;
    uint32_t first_block;                        // blockIdx.x of the item's first workgroup
};
static_assert(sizeof(SeedItem) == 24, "SeedItem is copied by words, and packed into the staging buffer");
// block_item[blockIdx.x]: index of the workgroup's item in the table the kernel is handed (as the batch kernels': sgd_batch.h).

// Seeds every stream of every item: d_items and d_block_item on the device, total_blocks = the sum of the items' workgroups
// (at most 2^31 - 1).  Asynchronous on st.
hipError_t seed_streams_device(const SeedItem *d_items, const uint32_t *d_block_item, uint32_t total_blocks, hipStream_t st);
hipError_t warm_module_set_setup();

}  // namespace gfs
