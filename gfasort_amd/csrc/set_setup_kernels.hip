// set_setup_kernels.hip — K3c: the RNG streams of every item of a context set, seeded in ONE launch (capi_set.hip setup_contexts:
// gfs_ctx_set_setup_*, and gfs_ctx_setup_* and gfs_ctx_reset_streams with a set of one).  On the host that is a loop of splitmix64
// over every stream of every item and a blocking copy per item.  Here the grid is the concatenation of
// the items' grids, as in the batch kernels (sgd_kernels_batch.hip): a workgroup looks its item up and never straddles two.
// 64-bit wrapping integer arithmetic throughout: the words are bit for bit the host's.
#include "set_seed.h"
#include "sgd_limits.h"

namespace gfs {

// Stream t of the workgroup's item <- Xoshiro256Plus::seed_from_u64(seed + stream_base + t) (sgd.rs:431-432): four successive
// splitmix64 outputs, word k to rng[k * n_streams + t] — for each k the lanes of a wave write 64 adjacent words.
// The item is read with scalar loads: its index comes from blockIdx alone, the two tables are written by the host before the
// launch and by nobody during it, so they are read through the constant address space as kernel arguments are
// (sgd_kernels_batch.hip load_item).  Plain vector stores, no atomics, no LDS.  The workgroup size is SEED_BLOCK, always.
__global__ void __launch_bounds__(SEED_BLOCK) set_seed_streams_kernel(const SeedItem *items, const uint32_t *block_item) {
    typedef const __attribute__((address_space(4))) uint32_t kword;
    const uint32_t idx = ((kword *)(uintptr_t)block_item)[blockIdx.x];
    kword *kw = (kword *)(uintptr_t)(items + idx);
    SeedItem it;
    uint32_t *dw = reinterpret_cast<uint32_t *>(&it);
    static_assert(sizeof(SeedItem) % 4 == 0, "SeedItem is copied by words");
#pragma unroll
    for (unsigned i = 0; i < sizeof(SeedItem) / 4; ++i) dw[i] = kw[i];
    const uint32_t t = (blockIdx.x - it.first_block) * SEED_BLOCK + threadIdx.x;
    if (t >= it.n_streams) return;                                         // the item's last workgroup
    uint64_t sm = it.first + t;
    // (a pointer read from memory is generic to the compiler: say that it is global, for global stores in place of flat ones)
    auto *rng = (__attribute__((address_space(1))) uint64_t *)(uintptr_t)it.rng;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) rng[(uint64_t)k * it.n_streams + t] = splitmix64(sm);
}

hipError_t seed_streams_device(const SeedItem *d_items, const uint32_t *d_block_item, uint32_t total_blocks, hipStream_t st) {
    if (!total_blocks) return hipSuccess;
    hipLaunchKernelGGL(set_seed_streams_kernel, dim3(total_blocks), dim3(SEED_BLOCK), 0, st, d_items, d_block_item);
    return hipGetLastError();
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_set_setup() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&set_seed_streams_kernel));
}

}  // namespace gfs
