// sgd_limits.h — the constants, the one plain structure and the seeding rule that the host code and the kernels share.  Free of HIP: the kernel
// headers (sgd_device.h, sgd_kernel_common.h, sgd_nd_team.h) include it in place of definitions of their own, and so do the
// host-only units (launch_policy.h, host_tables.hip), which a plain C++ compiler builds.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)     // __host__ __device__ __forceinline__, the last spelled out: a unit without the HIP runtime header lacks that macro
#define GFS_HOST_DEVICE __host__ __device__ inline __attribute__((always_inline))
#else
#define GFS_HOST_DEVICE inline
#endif

namespace gfs {

// ---- launch-uniform constants of one SGD batch (host-computed, bit-exact) ----------------
struct IterConsts {
    double   eta;          // etas[k]                                        sgd.rs:389,519
    double   zeta2theta;   // 1.0 + fpp(0.5, theta_cur)  (also the 2nd fast-path bound) :471,143
    double   omt_fb;       // (1 - theta_cur) split for fpp(2/n, 1-theta)               :133
    double   alpha_fb;     // alpha = 1/(1-theta_cur) split for fpp(.., alpha)          :132,148
    int32_t  omt_e;
    int32_t  alpha_e;
    int32_t  cooling;      // k > first_cooling_iteration                               :393-396
    int32_t  _pad;
};
// The host's form of sgd_device.h sat_i32 (Rust `as`: sgd.rs:149,157,164): it splits the exponents that IterConsts carries.
inline int32_t h_sat_i32(double v) {
    if (v != v) return 0;
    if (v <= -2147483648.0) return INT32_MIN;
    if (v >= 2147483647.0) return INT32_MAX;
    return (int32_t)v;
}

// rand_core's seed_from_u64: how every Xoshiro256+ state is seeded, the kernels' streams (sgd.rs:431-432), which are seeded on
// the device (set_setup_kernels.hip), and the host's generators (host_tables.hip) alike.
GFS_HOST_DEVICE uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint32_t COUNTER_SLOTS = 1024;    // counters: [COUNTER_SLOTS][8] u64, [s][0] = updates, [s][1] = attempts

// A team wave works through an iteration in CHUNKS of this many updates (sgd_kernel_common.h, work pools); the rank cut-off
// that makes a count exact applies at the end of every chunk.  2048 = 32 full trips.
constexpr uint32_t TEAM_CHUNK = 2048;        // (the value of KArgs.chunk unless a probe says otherwise: capi.hip gfs_ctx_run_range)
// ... and of this many in the layout kernels: their pool is ONE counter per iteration (sgd_kernels_nd_team.hip K2c), and half as many
// claims are worth 3 % (C4: 49.5 -> 51.0 G updates/s; 8192: 50.8; profiles/r03/chunk_size_probe.log).  The sort is best at 2048.
constexpr uint32_t ND_TEAM_CHUNK = 4096;

// Work pools (sgd_kernel_common.h pool_walk has the why and the measurements).
constexpr uint32_t POOL_SLOTS = 16, POOL_STRIDE = 16;              // counters per iteration; u32 per 64-B line
// Counters in use: one per 16 waves, at most POOL_SLOTS.  Several counters exist so that 4 000 waves do not queue on one
// address; a counter must still be SHARED by many waves — a wave with a counter of its own has a fixed quota again and drifts
// away from the others in the schedule (a 40-lane last wave beside 15 full ones, each on its own counter, ran 60 % behind and
// cost DRB1 a fifth of its final stress: 0.39 against 0.33, round 3).
GFS_HOST_DEVICE uint32_t pool_slots(uint32_t n_waves) {
    const uint32_t s = n_waves / 16u;
    return s < 1u ? 1u : (s > POOL_SLOTS ? POOL_SLOTS : s);
}
// the zeroed counters a pooled fused launch over n_iters iterations draws from
inline size_t pool_bytes(uint64_t n_iters) { return (size_t)n_iters * POOL_SLOTS * POOL_STRIDE * sizeof(uint32_t); }

// K1d / K2d: updates per live lane and pool claim (sgd_kernel_common.h ref_pooled_walk)
constexpr uint32_t REF_CHUNK_PER_LANE = 16;

// Waves per SIMD the layout team kernels (sgd_nd_team.h) are built for.
// (3 waves per SIMD, <= 168 VGPRs: 165 at D = 2, nothing spilled; D = 3: two waves, 176, see nd_waves_for.  Round 2's kernel needed ~210 and ran
// two waves — a twin trip holds the records of three steps and of the steps after them, the next trip's too, and three ends'
// coordinates.  What brought it under 168: the trip machine's state in scalar registers (uni), steps as 32-bit ranks in their
// path, no lane permutes for the adds (dimension planes), the sampler's constants re-read per pass.  Three waves hide the
// round trip of a trip's loads and adds behind two other waves' arithmetic: without the adds the kernel runs at 64 G updates/s
// where two waves gave 51 (profiles/r03/nd_waves3.log).  Hence also the bound on the workgroup size, checked by the host.)
#ifndef GFS_ND_TEAM_WAVES
#define GFS_ND_TEAM_WAVES 3
#endif
// (D = 3 holds half as many coordinates again: three waves' worth of registers spill 4-11 of them, and under the work pool two
// waves are as fast — 34.2 against 34.3 G updates/s on C4, profiles/r03/nd_k_probe_fused.log — so D = 3 is built for two.  So is every
// wider layout: two waves leave 256 VGPRs, enough for D = 8 without spilling, the trace kernel at B = 64 using all of them.)
constexpr int nd_waves_for(int dims) { return dims >= 3 ? 2 : GFS_ND_TEAM_WAVES; }
inline int nd_team_waves(int dims) { return nd_waves_for(dims); }

}  // namespace gfs
