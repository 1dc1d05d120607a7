// sgd_kernels_batch.hip — K1f / K2f: the fused reference-stream kernels (K1d, sgd_kernels_1d.hip; K2d, sgd_kernels_nd.hip) over
// MANY graphs in one persistent launch.  A graph below 16 384 nodes runs at most one stream per 4 nodes (launch_policy.h
// auto_stream_count): DRB1-3123 is 5 workgroups, and nothing done within the graph fills the other 250 CUs.  Here the grid is the
// concatenation of the items' grids; a workgroup looks its item up, and from there on it is K1d / K2d on that item's buffers.
#include "sgd_1d.h"
#include "sgd_nd.h"
#include "sgd_batch.h"
#include "sgd_host.h"

namespace gfs {

// A workgroup's item, read from the table with scalar loads: the index comes from blockIdx alone, the table is written by the host
// before the launch and by nobody during it, so it is read through the constant address space as the kernel arguments are
// (sgd_kernel_common.h reload_kargs).  KArgs, its, n_iters and pool are then in scalar registers exactly as K1d's arguments are.
__device__ __forceinline__ void load_item(const BatchItem *items, const uint32_t *block_item, BatchItem &it) {
    typedef const __attribute__((address_space(4))) uint32_t kword;
    const uint32_t idx = ((kword *)(uintptr_t)block_item)[blockIdx.x];
    kword *kw = (kword *)(uintptr_t)(items + idx);
    uint32_t *dw = reinterpret_cast<uint32_t *>(&it);
    static_assert(sizeof(BatchItem) % 4 == 0, "BatchItem is copied by words");
#pragma unroll
    for (unsigned i = 0; i < sizeof(BatchItem) / 4; ++i) dw[i] = kw[i];
}

// K1f: K1d's body on the item of this workgroup.  tid, and with it the wave index that pool_share sees, counts from the item's
// first workgroup; flush_counters takes its slot from the global index (the counters are summed: any slot is right).
template <bool LDS_TABLES>
__global__ void sgd1d_batch_fused_kernel(const BatchItem *items, const uint32_t *block_item) {
    extern __shared__ __align__(16) unsigned char smem[];
    BatchItem it;
    load_item(items, block_item, it);
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(it.a, smem, path_tab, zeta_tab);
    const uint32_t tid = (blockIdx.x - it.first_block) * blockDim.x + threadIdx.x;
    if ((tid & ~63u) >= it.a.n_streams) return;                        // waves without a live lane
    const bool live = tid < it.a.n_streams;
    KArgs a = it.a;
    Rng rng = {0, 0, 0, 0};
    if (live) load_rng(a, tid, rng);
    uint32_t done = 0, att = 0, ntr = 0;
    ref_pooled_walk(a, it.its, it.n_iters, it.pool, tid, [&](const uint32_t share, const uint64_t max_att) {
        ref_run_1d<LDS_TABLES, true, false>(a, path_tab, zeta_tab, rng, share, max_att, tid, done, att, ntr);
    });
    if (live) store_rng(a, tid, rng);
    flush_counters(a, done, att);
}

// K2f: the same over K2d's body (ref_run_nd), D = 2 and 3: the layouts the command line makes.
template <int D, bool LDS_TABLES>
__global__ void sgdnd_batch_fused_kernel(const BatchItem *items, const uint32_t *block_item) {
    extern __shared__ __align__(16) unsigned char smem[];
    BatchItem it;
    load_item(items, block_item, it);
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(it.a, smem, path_tab, zeta_tab);
    const uint32_t tid = (blockIdx.x - it.first_block) * blockDim.x + threadIdx.x;
    if ((tid & ~63u) >= it.a.n_streams) return;
    const bool live = tid < it.a.n_streams;
    KArgs a = it.a;
    Rng rng = {0, 0, 0, 0};
    if (live) load_rng(a, tid, rng);
    uint32_t done = 0, att = 0, ntr = 0;
    ref_pooled_walk(a, it.its, it.n_iters, it.pool, tid, [&](const uint32_t share, const uint64_t max_att) {
        ref_run_nd<D, LDS_TABLES, true, false>(a, path_tab, zeta_tab, rng, share, max_att, tid, done, att, ntr);
    });
    if (live) store_rng(a, tid, rng);
    flush_counters(a, done, att);
}

const void *batch_fused_kernel(int dims, bool lds_tables) {
    switch (dims) {
        case 0: return with_flag(lds_tables, [](auto L) { return kernel_addr(sgd1d_batch_fused_kernel<L()>); });
        case 2: return with_flag(lds_tables, [](auto L) { return kernel_addr(sgdnd_batch_fused_kernel<2, L()>); });
        case 3: return with_flag(lds_tables, [](auto L) { return kernel_addr(sgdnd_batch_fused_kernel<3, L()>); });
        default: return nullptr;
    }
}

}  // namespace gfs
