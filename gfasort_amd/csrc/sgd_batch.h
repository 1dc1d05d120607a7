// sgd_batch.h — the two tables a batch launch reads (sgd_kernels_batch.hip; written by capi_batch.hip gfs_batch_run).
#pragma once
#include "sgd_device.h"

namespace gfs {

// One context of the batch: what K1d / K2d take as kernel arguments, and where its grid starts in the launch's.
struct BatchItem {
    KArgs a;                       // as fill_kargs makes them, a.it = the constants of iteration 0
    const IterConsts *its;         // the context's resident schedule
    uint32_t *pool;                // n_iters * POOL_SLOTS counters, zeroed before the launch
    uint32_t n_iters;
    uint32_t first_block;          // blockIdx.x of the item's first workgroup
};
// block_item[blockIdx.x]: index of the workgroup's item in the table the kernel is handed.

}  // namespace gfs
