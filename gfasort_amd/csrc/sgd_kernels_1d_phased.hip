// sgd_kernels_1d_phased.hip — K1e: the PHASED sampler of the 1D sort (GFS_F_PHASED), one persistent pooled launch over any
// range of iterations.  An iteration is either a TEAM iteration (K1c's trip machine at B = 64, team_iteration) or a WINDOW
// iteration (every lane is reference stream `tid`, K1d's ref_run_1d): the host marks the window's iterations in IterConsts._pad
// (launch_policy.h iter_consts), and every wave reads the mark with the iteration's constants — a scalar load, a wave-uniform branch.
// Both samplers draw from the same per-lane RNG in registers, and each continues the state the other left; a team pass left
// over when a window begins is kept and dropped by the team's own rule (a cooling flag other than the one it was sampled
// under).  That is the oracle with gfo_state_set_bundle switched between 64 and 1 between iterations.
// The device functions are sgd_1d.h's, shared with K1 / K1b / K1c / K1d.
#include "sgd_1d.h"
#include "sgd_host.h"

namespace gfs {

// The work pools of K1c / K1d (sgd_kernel_common.h pool_walk): iteration k's updates are claimed from its own counters, in chunks
// of TEAM_CHUNK updates per wave in a team iteration and of REF_CHUNK_PER_LANE per lane in a window iteration (each drawn dry
// before the wave moves on, so every iteration applies exactly its updates).  The first claim of iteration k + 1 is sized by
// k + 1's own sampler, not by k's: one wave is bit for bit K1d in a window iteration and K1c in a team iteration (tested), and
// each works through an iteration in its own chunks.
// (4 waves per SIMD, as K1c: the trip machine needs its 128 VGPRs; ref_run_1d needs far fewer.)
template <bool LDS_TABLES>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) sgd1d_phased_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters,
                                                                                     uint32_t *pool) {
    constexpr int B = 64;
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a0, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;       // n_streams % 64 == 0 (host-checked): whole waves
    if (tid >= a0.n_streams) return;
    KArgs a = a0;
    TeamState ts;
    uint32_t no_flips = 0;                                            // (the sort has no end flips)
    load_rng(a, tid, ts.rng);
    const uint32_t lane = threadIdx.x & 63u;
    load_pass(a, tid, ts, no_flips);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (scalar registers)
    const uint32_t ref_chunk = 64u * a0.ref_chunk;                    // K1d's chunk of a wave of 64 live lanes
    // pool_walk's loop written out — KEEP IN STEP with sgd_kernel_common.h pool_walk.  (Through the helper the LDS_TABLES build,
    // the one a graph whose tables fit the LDS gets, spills 35 scalar registers to lanes instead of 29; the build without them
    // 42 instead of 53.  Both then take 128 VGPRs instead of 127, and the same 12 B of scratch.)
    const PoolShare ps = pool_share(a0, wave, a0.n_streams >> 6);
    uint32_t k = 0, claim = 0;
    a.it = its[0];
    uint32_t chunk = a.it._pad ? ref_chunk : a0.chunk;
    send_claim(pool + ps.slot * POOL_STRIDE, chunk, claim);
    while (k < n_iters) {
        const uint32_t old = (uint32_t)__builtin_amdgcn_readfirstlane((int)claim);
        if (old >= ps.cap) {                                           // this iteration's pool is exhausted
            if (++k == n_iters) break;
            a.it = its[k];                                             // wave-uniform: scalar loads
            chunk = a.it._pad ? ref_chunk : a0.chunk;                  // the first claim of an iteration is sized by its sampler
            send_claim(pool + ((size_t)k * POOL_SLOTS + ps.slot) * POOL_STRIDE, chunk, claim);
            continue;
        }
        send_claim(pool + ((size_t)k * POOL_SLOTS + ps.slot) * POOL_STRIDE, chunk, claim);   // travels while this chunk is worked on
        const uint32_t m = ps.cap - old < chunk ? ps.cap - old : chunk;
        if (__builtin_expect(a.it._pad != 0, 0)) {                                               // window: reference streams, K1d's equal shares
            // (the launch constants read afresh, as the team sampler does — sgd_kernel_common.h reload_kargs: held through the
            // trip machine as well, they spilled 49 scalar registers and 10 vector ones into scratch)
            KArgs as;
            reload_kargs(as);
            as.it = a.it;
            const uint32_t share = m / 64u + (lane < m % 64u ? 1u : 0u);
            if (share) ref_run_1d<LDS_TABLES, true, false>(as, path_tab, zeta_tab, ts.rng, share, (uint64_t)as.attempt_factor * share + 64u,
                                                           tid, ts.done, ts.att, ts.ntr);
        } else {
            team_iteration<B, LDS_TABLES, true, false>(a, path_tab, zeta_tab, ts, tid, m, its + k);
        }
    }
    // (the exit addresses are derived afresh: kept from the entry's loads they were spilled to scratch for the whole launch)
    uint32_t te = tid;
    asm volatile("" : "+v"(te));
    store_rng(a, te, ts.rng);
    store_pass(a, te, ts, 0u);
    flush_counters(a, ts.done, ts.att);
}

// (the phased launch is always pooled)
const void *phased_fused_kernel(bool lds_tables) {
    return with_flag(lds_tables, [](auto L) { return kernel_addr(sgd1d_phased_fused_kernel<L()>); });
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_1d_phased() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sgd1d_phased_fused_kernel<true>));
}

}  // namespace gfs
