// sgd_kernels_nd.hip — K2: reference-stream kernels of path_linear_sgd_layout, D = 1..8.
#include "sgd_nd.h"
#include "sgd_host.h"

namespace gfs {

// ------------------------------------------------------------------------------------------
// K2: nD, D compile-time.  coords in planes [end][dim][slot] (sgd_device.h coord_ptr); the trace
// speaks the reference's index 2*node+end (sgd.rs:1099-1103).  The streams' loop is ref_run_nd (sgd_nd.h).
// ------------------------------------------------------------------------------------------
template <int D, bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE>
__global__ void sgdnd_kernel(const KArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a, smem, path_tab, zeta_tab);

    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = tid < a.n_streams;
    uint32_t done = 0, att = 0;
    if (live) {
        Rng rng;
        load_rng(a, tid, rng);
        const uint32_t quota = a.quota_base + (tid < a.quota_rem ? 1u : 0u);
        const uint64_t max_att64 = (uint64_t)a.attempt_factor * quota + 1024u;
        const uint64_t max_att = max_att64 > 0xFFFFFFFFull ? 0xFFFFFFFFull : max_att64;
        uint32_t ntr = TRACE ? a.trace_cnt[tid] : 0;
        ref_run_nd<D, LDS_TABLES, ATOMIC_LOADS, TRACE>(a, path_tab, zeta_tab, rng, quota, max_att, tid, done, att, ntr);
        store_rng(a, tid, rng);
        if (TRACE) a.trace_cnt[tid] = ntr;
    }
    flush_counters(a, done, att);
}

// K2d: the same streams, a range of iterations in one persistent launch with work pools (sgd_kernel_common.h
// ref_pooled_walk, pool_walk; K1d in sgd_kernels_1d.hip is the 1D form).
template <int D, bool LDS_TABLES>
__global__ void sgdnd_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters, uint32_t *pool) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a0, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if ((tid & ~63u) >= a0.n_streams) return;                          // waves without a live lane
    const bool live = tid < a0.n_streams;
    KArgs a = a0;
    Rng rng = {0, 0, 0, 0};
    if (live) load_rng(a, tid, rng);
    uint32_t done = 0, att = 0, ntr = 0;
    ref_pooled_walk(a, its, n_iters, pool, tid, [&](const uint32_t share, const uint64_t max_att) {
        ref_run_nd<D, LDS_TABLES, true, false>(a, path_tab, zeta_tab, rng, share, max_att, tid, done, att, ntr);
    });
    if (live) store_rng(a, tid, rng);
    flush_counters(a, done, att);
}

template <int D>
static const void *kernel_nd(const KernelShape &s) {
    return with_flag(s.lds_tables, [&](auto L) { return with_flag(s.atomic_loads, [&](auto A) { return with_flag(s.trace, [&](auto T) {
        return kernel_addr(sgdnd_kernel<D, L(), A(), T()>);
    }); }); });
}
template <int D>
static const void *fused_kernel_nd(bool lds_tables) {
    return with_flag(lds_tables, [](auto L) { return kernel_addr(sgdnd_fused_kernel<D, L()>); });
}
const void *iteration_kernel_nd(const KernelShape &s) {
    switch (s.dims) {
        case 1: return kernel_nd<1>(s);
        case 2: return kernel_nd<2>(s);
        case 3: return kernel_nd<3>(s);
        case 4: return kernel_nd<4>(s);
        case 5: return kernel_nd<5>(s);
        case 6: return kernel_nd<6>(s);
        case 7: return kernel_nd<7>(s);
        case 8: return kernel_nd<8>(s);
        default: return nullptr;
    }
}
// reference streams, fused (K2d): pooled only
const void *fused_kernel_nd(const KernelShape &s, bool pooled) {
    if (!pooled) return nullptr;
    switch (s.dims) {
        case 1: return fused_kernel_nd<1>(s.lds_tables);
        case 2: return fused_kernel_nd<2>(s.lds_tables);
        case 3: return fused_kernel_nd<3>(s.lds_tables);
        case 4: return fused_kernel_nd<4>(s.lds_tables);
        case 5: return fused_kernel_nd<5>(s.lds_tables);
        case 6: return fused_kernel_nd<6>(s.lds_tables);
        case 7: return fused_kernel_nd<7>(s.lds_tables);
        case 8: return fused_kernel_nd<8>(s.lds_tables);
        default: return nullptr;
    }
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_nd() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgdnd_kernel<2, true, true, false>));
}

}  // namespace gfs
