// sgd_kernels_nd_team_wide.hip — K2b / K2c for layouts of D = 4..8 dimensions: the templates of sgd_nd_team.h, the same trip
// machine as D = 2, 3 (runs of GFS_F_CHAIN trips, one set of end flips per run, two partners per leader with twin trips, fused
// short-jump trips with one add per end), instantiated in a translation unit of their own so that they compile beside D = 1..3.
// Built for two waves per SIMD (nd_waves_for): 192-246 VGPRs for the fused kernels, 256 for the D = 8 trace kernel at B = 64,
// nothing spilled (profiles/r04/nd_wide_resource_usage.txt).  The auto policy does not pick them (launch_policy.h choose_bundle):
// they are reached with an explicit GFS_F_BUNDLE(8..64).
#include "sgd_nd_team.h"

namespace gfs {

const void *iteration_kernel_nd_team_wide(const KernelShape &s) {
#define GFS_NDB_CASE(D, B) if (s.dims == D && s.bundle == B) return team_kernel_nd<D, B>(s);
    GFS_NDB_CASE(4, 8) GFS_NDB_CASE(4, 16) GFS_NDB_CASE(4, 32) GFS_NDB_CASE(4, 64)
    GFS_NDB_CASE(5, 8) GFS_NDB_CASE(5, 16) GFS_NDB_CASE(5, 32) GFS_NDB_CASE(5, 64)
    GFS_NDB_CASE(6, 8) GFS_NDB_CASE(6, 16) GFS_NDB_CASE(6, 32) GFS_NDB_CASE(6, 64)
    GFS_NDB_CASE(7, 8) GFS_NDB_CASE(7, 16) GFS_NDB_CASE(7, 32) GFS_NDB_CASE(7, 64)
    GFS_NDB_CASE(8, 8) GFS_NDB_CASE(8, 16) GFS_NDB_CASE(8, 32) GFS_NDB_CASE(8, 64)
#undef GFS_NDB_CASE
    return nullptr;
}

const void *fused_kernel_nd_team_wide(const KernelShape &s, bool pooled) {
    switch (s.dims) {
    case 4: return team_fused_kernel_nd<4>(s, pooled);
    case 5: return team_fused_kernel_nd<5>(s, pooled);
    case 6: return team_fused_kernel_nd<6>(s, pooled);
    case 7: return team_fused_kernel_nd<7>(s, pooled);
    case 8: return team_fused_kernel_nd<8>(s, pooled);
    default: return nullptr;
    }
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_nd_team_wide() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgdnd_team_fused_kernel<4, 64, true, true>));
}

}  // namespace gfs
