// sgd_kernels_1d_phased.hip — K1e: the PHASED sampler of the 1D sort (GFS_F_PHASED), one persistent pooled launch over any
// range of iterations.  An iteration is either a TEAM iteration (K1c's trip machine at B = 64, team_iteration) or a WINDOW
// iteration (every lane is reference stream `tid`, K1d's ref_run_1d): the host marks the window's iterations in IterConsts._pad
// (capi.hip iter_consts), and every wave reads the mark with the iteration's constants — a scalar load, a wave-uniform branch.
// Both samplers draw from the same per-lane RNG in registers, and each continues the state the other left; a team pass left
// over when a window begins is kept and dropped by the team's own rule (a cooling flag other than the one it was sampled
// under).  That is the oracle with gfo_state_set_bundle switched between 64 and 1 between iterations.
// The device functions are sgd_1d.h's, shared with K1 / K1b / K1c / K1d.
#include "sgd_1d.h"
#include "sgd_host.h"

namespace gfs {

// The work pools of K1c / K1d (sgd_kernel_common.h): iteration k's updates are claimed from its own counters, in chunks of
// TEAM_CHUNK updates per wave in a team iteration and of REF_CHUNK_PER_LANE per lane in a window iteration (each drawn dry
// before the wave moves on, so every iteration applies exactly its updates).  The claim a wave sends ahead is always for the
// iteration it works in; the first claim of iteration k + 1 is sized by k + 1's own sampler.
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
    const uint64_t T = a0.n_streams;
    KArgs a = a0;
    TeamState ts;
    ts.rng.s0 = a.rng[tid]; ts.rng.s1 = a.rng[T + tid]; ts.rng.s2 = a.rng[2 * T + tid]; ts.rng.s3 = a.rng[3 * T + tid];
    const uint32_t lane = threadIdx.x & 63u;
    load_pass(a, tid, ts);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), n_waves = a0.n_streams >> 6;   // (scalar registers)
    const uint32_t slots = pool_slots(n_waves), slot = wave % slots;
    const uint64_t total = (uint64_t)a0.quota_base * a0.n_streams + a0.quota_rem;
    const uint32_t cap = (uint32_t)(total / slots + (slot < total % slots ? 1u : 0u));   // < 2^31 (host-checked)
    const uint32_t ref_chunk = 64u * a0.ref_chunk;                    // K1d's chunk of a wave of 64 live lanes
    uint32_t k = 0, claim = 0;
    a.it = its[0];
    uint32_t chunk = a.it._pad ? ref_chunk : a0.chunk;
    if (lane == 0) claim = __hip_atomic_fetch_add(pool + slot * POOL_STRIDE, chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (k < n_iters) {
        const uint32_t old = (uint32_t)__builtin_amdgcn_readfirstlane((int)claim);
        if (old >= cap) {                                              // this iteration's pool is exhausted
            if (++k == n_iters) break;
            a.it = its[k];                                             // wave-uniform: scalar loads
            chunk = a.it._pad ? ref_chunk : a0.chunk;                  // the first claim of an iteration is sized by its sampler
            if (lane == 0) claim = __hip_atomic_fetch_add(pool + ((size_t)k * POOL_SLOTS + slot) * POOL_STRIDE, chunk,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        // the next claim travels while this chunk is worked on
        if (lane == 0) claim = __hip_atomic_fetch_add(pool + ((size_t)k * POOL_SLOTS + slot) * POOL_STRIDE, chunk,
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t m = cap - old < chunk ? cap - old : chunk;
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
    a.rng[te] = ts.rng.s0; a.rng[T + te] = ts.rng.s1; a.rng[2 * T + te] = ts.rng.s2; a.rng[3 * T + te] = ts.rng.s3;
    store_pass(a, te, ts);
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
