// sgd_kernels_nd_team.hip — K2b / K2c for D = 1..3 (one launch per iteration; the fused pooled launch of a range of iterations
// for D = 2, 3 at B = 64).  The kernel templates are in sgd_nd_team.h; D = 4..8 are instantiated in
// sgd_kernels_nd_team_wide.hip.
#include "sgd_nd_team.h"

namespace gfs {

const void *iteration_kernel_nd_team(const KernelShape &s) {
#define GFS_NDB_CASE(D, B) if (s.dims == D && s.bundle == B) return team_kernel_nd<D, B>(s);
    GFS_NDB_CASE(1, 8) GFS_NDB_CASE(1, 16) GFS_NDB_CASE(1, 32) GFS_NDB_CASE(1, 64)
    GFS_NDB_CASE(2, 8) GFS_NDB_CASE(2, 16) GFS_NDB_CASE(2, 32) GFS_NDB_CASE(2, 64)
    GFS_NDB_CASE(3, 8) GFS_NDB_CASE(3, 16) GFS_NDB_CASE(3, 32) GFS_NDB_CASE(3, 64)
#undef GFS_NDB_CASE
    return nullptr;
}

// K2c: layouts of 2 and more dimensions at B = 64 (what the auto policy picks on graphs large enough for it to matter,
// for D = 2, 3)
const void *fused_kernel_nd_team(const KernelShape &s, bool pooled) {
    if (s.dims == 2) return team_fused_kernel_nd<2>(s, pooled);
    if (s.dims == 3) return team_fused_kernel_nd<3>(s, pooled);
    return nullptr;
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_nd_team() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgdnd_team_kernel<2, 64, true, true, false>));
}

}  // namespace gfs
