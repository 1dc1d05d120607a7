// sgd_kernels_nd_team_wide.hip — K2b / K2c for layouts of D = 4..8 dimensions: the templates of sgd_nd_team.h, the same trip
// machine as D = 2, 3 (runs of GFS_F_CHAIN trips, one set of end flips per run, two partners per leader with twin trips, fused
// short-jump trips with one add per end), instantiated in a translation unit of their own so that they compile beside D = 1..3.
// Built for two waves per SIMD (nd_waves_for): 192-246 VGPRs for the fused kernels, 256 for the D = 8 trace kernel at B = 64,
// nothing spilled (profiles/r04/nd_wide_resource_usage.txt).  The auto policy does not pick them (capi.hip choose_bundle):
// they are reached with an explicit GFS_F_BUNDLE(8..64).
#include "sgd_nd_team.h"

namespace gfs {

hipError_t launch_nd_team_wide(int dims, const KArgs &a, bool lds_tables, bool trace, dim3 grid, dim3 block, size_t lds, hipStream_t st) {
#define GFS_NDB_CASE(D, B) if (dims == D && a.bundle == B) return launch_ndb<D, B>(a, lds_tables, true, trace, grid, block, lds, st);
    GFS_NDB_CASE(4, 8) GFS_NDB_CASE(4, 16) GFS_NDB_CASE(4, 32) GFS_NDB_CASE(4, 64)
    GFS_NDB_CASE(5, 8) GFS_NDB_CASE(5, 16) GFS_NDB_CASE(5, 32) GFS_NDB_CASE(5, 64)
    GFS_NDB_CASE(6, 8) GFS_NDB_CASE(6, 16) GFS_NDB_CASE(6, 32) GFS_NDB_CASE(6, 64)
    GFS_NDB_CASE(7, 8) GFS_NDB_CASE(7, 16) GFS_NDB_CASE(7, 32) GFS_NDB_CASE(7, 64)
    GFS_NDB_CASE(8, 8) GFS_NDB_CASE(8, 16) GFS_NDB_CASE(8, 32) GFS_NDB_CASE(8, 64)
#undef GFS_NDB_CASE
    return hipErrorInvalidValue;
}

hipError_t launch_nd_team_fused_wide(int dims, const KArgs &a, const IterConsts *d_its, uint32_t n_iters, bool lds_tables, uint32_t *pool,
                                     dim3 grid, dim3 block, size_t lds, hipStream_t st) {
    switch (dims) {
    case 4: return launch_nd_team_fused_d<4>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    case 5: return launch_nd_team_fused_d<5>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    case 6: return launch_nd_team_fused_d<6>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    case 7: return launch_nd_team_fused_d<7>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    case 8: return launch_nd_team_fused_d<8>(a, d_its, n_iters, lds_tables, pool, grid, block, lds, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t prepare_nd_team_fused_wide(int dims, bool lds_tables, int block, size_t lds, int *blocks_per_cu) {
    switch (dims) {
    case 4: return prepare_nd_team_fused_d<4>(lds_tables, block, lds, blocks_per_cu);
    case 5: return prepare_nd_team_fused_d<5>(lds_tables, block, lds, blocks_per_cu);
    case 6: return prepare_nd_team_fused_d<6>(lds_tables, block, lds, blocks_per_cu);
    case 7: return prepare_nd_team_fused_d<7>(lds_tables, block, lds, blocks_per_cu);
    case 8: return prepare_nd_team_fused_d<8>(lds_tables, block, lds, blocks_per_cu);
    default: *blocks_per_cu = 0; return hipSuccess;
    }
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_nd_team_wide() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgdnd_team_fused_kernel<4, 64, true, true>));
}

}  // namespace gfs
