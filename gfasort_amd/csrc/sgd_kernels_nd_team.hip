// sgd_kernels_nd_team.hip — K2b / K2c for D = 1..3 (one launch per iteration; the fused pooled launch of a range of iterations
// for D = 2, 3 at B = 64) and the nD launch dispatcher.  The kernel templates are in sgd_nd_team.h; D = 4..8 are instantiated in
// sgd_kernels_nd_team_wide.hip.
#include "sgd_nd_team.h"

namespace gfs {

hipError_t launch_nd_ref(int dims, const KArgs &a, bool lds_tables, bool atomic_loads, bool trace,
                         dim3 grid, dim3 block, size_t lds, hipStream_t st);
// sgd_kernels_nd_team_wide.hip: the same for D = 4..8
hipError_t launch_nd_team_wide(int dims, const KArgs &a, bool lds_tables, bool trace, dim3 grid, dim3 block, size_t lds, hipStream_t st);
hipError_t launch_nd_team_fused_wide(int dims, const KArgs &a, const IterConsts *d_its, uint32_t n_iters, bool lds_tables, uint32_t *pool,
                                     dim3 grid, dim3 block, size_t lds, hipStream_t st);
hipError_t prepare_nd_team_fused_wide(int dims, bool lds_tables, int block, size_t lds, int *blocks_per_cu);


hipError_t launch_nd(int dims, const KArgs &a, bool lds_tables, bool atomic_loads, bool trace,
                     dim3 grid, dim3 block, size_t lds, hipStream_t st) {
    if (dims >= 1 && dims <= 3 && a.bundle >= 8) {
#define GFS_NDB_CASE(D, B) if (dims == D && a.bundle == B) return launch_ndb<D, B>(a, lds_tables, atomic_loads, trace, grid, block, lds, st);
        GFS_NDB_CASE(1, 8) GFS_NDB_CASE(1, 16) GFS_NDB_CASE(1, 32) GFS_NDB_CASE(1, 64)
        GFS_NDB_CASE(2, 8) GFS_NDB_CASE(2, 16) GFS_NDB_CASE(2, 32) GFS_NDB_CASE(2, 64)
        GFS_NDB_CASE(3, 8) GFS_NDB_CASE(3, 16) GFS_NDB_CASE(3, 32) GFS_NDB_CASE(3, 64)
#undef GFS_NDB_CASE
    }
    if (dims >= 4 && dims <= 8 && a.bundle >= 8) return launch_nd_team_wide(dims, a, lds_tables, trace, grid, block, lds, st);
    return launch_nd_ref(dims, a, lds_tables, atomic_loads, trace, grid, block, lds, st);
}

// K2c launchers: layouts of 2 and more dimensions at B = 64 (what the auto policy picks on graphs large enough for it to matter,
// for D = 2, 3).
hipError_t launch_nd_team_fused(int dims, const KArgs &a, const IterConsts *d_its, uint32_t n_iters, bool lds_tables, uint32_t *pool,
                                dim3 grid, dim3 block, size_t lds, hipStream_t st) {
    if (a.bundle != 64u) return hipErrorInvalidValue;
    if (dims == 2) return launch_nd_team_fused_d<2>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    if (dims == 3) return launch_nd_team_fused_d<3>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    if (dims >= 4 && dims <= 8) return launch_nd_team_fused_wide(dims, a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    return hipErrorInvalidValue;
}
// workgroups of the fused kernel one CU holds at once (0: no fused kernel for this shape)
hipError_t prepare_nd_team_fused(int dims, uint32_t bundle, bool lds_tables, int block, size_t lds, int *blocks_per_cu) {
    *blocks_per_cu = 0;
    if (bundle != 64u) return hipSuccess;
    if (dims == 2) return prepare_nd_team_fused_d<2>(lds_tables, block, lds, blocks_per_cu);
    if (dims == 3) return prepare_nd_team_fused_d<3>(lds_tables, block, lds, blocks_per_cu);
    if (dims >= 4 && dims <= 8) return prepare_nd_team_fused_wide(dims, lds_tables, block, lds, blocks_per_cu);
    return hipSuccess;
}

// waves per SIMD the layout team kernels are built for (the host sizes the stream count by it)
int nd_team_waves(int dims) { return nd_waves_for(dims); }

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_nd_team() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgdnd_team_kernel<2, 64, true, true, false>));
}

}  // namespace gfs
