// sgd_kernels_1d.hip — K1 (reference streams) and K1b (team kernel) of path_linear_sgd, plus the
// multi-GPU replica-merge kernels.  See sgd_kernel_common.h / sgd_device.h.
#include "sgd_1d.h"
#include "sgd_host.h"

namespace gfs {

// K1: reference streams, one launch per iteration (ref_run_1d: sgd_1d.h)
template <bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE>
__global__ void sgd1d_kernel(const KArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a, smem, path_tab, zeta_tab);

    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = tid < a.n_streams;
    uint32_t done = 0, att = 0;
    if (live) {
        Rng rng;
        const uint64_t T = a.n_streams;
        rng.s0 = a.rng[tid]; rng.s1 = a.rng[T + tid]; rng.s2 = a.rng[2 * T + tid]; rng.s3 = a.rng[3 * T + tid];
        const uint32_t quota = a.quota_base + (tid < a.quota_rem ? 1u : 0u);
        const uint64_t max_att64 = (uint64_t)a.attempt_factor * quota + 1024u;
        const uint64_t max_att = max_att64 > 0xFFFFFFFFull ? 0xFFFFFFFFull : max_att64;
        uint32_t ntr = TRACE ? a.trace_cnt[tid] : 0;
        ref_run_1d<LDS_TABLES, ATOMIC_LOADS, TRACE>(a, path_tab, zeta_tab, rng, quota, max_att, tid, done, att, ntr);
        a.rng[tid] = rng.s0; a.rng[T + tid] = rng.s1; a.rng[2 * T + tid] = rng.s2; a.rng[3 * T + tid] = rng.s3;
        if (TRACE) a.trace_cnt[tid] = ntr;
    }
    flush_counters(a, done, att);
}

// K1d: the same streams, a range of iterations in one persistent launch with work pools (sgd_kernel_common.h
// ref_pooled_walk).  RNG state stays in registers for the whole schedule.
template <bool LDS_TABLES>
__global__ void sgd1d_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters, uint32_t *pool) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a0, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if ((tid & ~63u) >= a0.n_streams) return;                          // waves without a live lane
    const bool live = tid < a0.n_streams;
    const uint64_t T = a0.n_streams;
    KArgs a = a0;
    Rng rng = {0, 0, 0, 0};
    if (live) { rng.s0 = a.rng[tid]; rng.s1 = a.rng[T + tid]; rng.s2 = a.rng[2 * T + tid]; rng.s3 = a.rng[3 * T + tid]; }
    uint32_t done = 0, att = 0, ntr = 0;
    ref_pooled_walk(a, its, n_iters, pool, tid, [&](const uint32_t share, const uint64_t max_att) {
        ref_run_1d<LDS_TABLES, true, false>(a, path_tab, zeta_tab, rng, share, max_att, tid, done, att, ntr);
    });
    if (live) { a.rng[tid] = rng.s0; a.rng[T + tid] = rng.s1; a.rng[2 * T + tid] = rng.s2; a.rng[3 * T + tid] = rng.s3; }
    flush_counters(a, done, att);
}


// (4 waves per SIMD = 128 VGPRs: a twin trip keeps three blocks in flight and the next trip's records are on their way; built
// for 5 waves — 96 VGPRs — the kernel spills 58 registers and is slower: 88.5 against 91.5 G updates/s on C3 with round 1's
// launch, profiles/r02/two_partners.log.  Before the twin trips a fifth wave was worth +3 %.)
template <int B, bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) sgd1d_team_kernel(const KArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;       // n_streams % 64 == 0 (host-checked)
    if (tid >= a.n_streams) return;                                   // whole waves only
    const uint64_t T = a.n_streams;
    TeamState ts;
    ts.rng.s0 = a.rng[tid]; ts.rng.s1 = a.rng[T + tid]; ts.rng.s2 = a.rng[2 * T + tid]; ts.rng.s3 = a.rng[3 * T + tid];
    ts.ntr = TRACE ? a.trace_cnt[tid] : 0;
    load_pass(a, tid, ts);
    const uint64_t wq = wave_quota_of(a, tid);                        // worked through in chunks, like a pool (K1c)
    for (uint64_t done = 0; done < wq; done += a.chunk)
        team_iteration<B, LDS_TABLES, ATOMIC_LOADS, TRACE>(a, path_tab, zeta_tab, ts, tid, wq - done < a.chunk ? wq - done : a.chunk);
    a.rng[tid] = ts.rng.s0; a.rng[T + tid] = ts.rng.s1; a.rng[2 * T + tid] = ts.rng.s2; a.rng[3 * T + tid] = ts.rng.s3;
    if (TRACE) a.trace_cnt[tid] = ts.ntr;
    store_pass(a, tid, ts);
    flush_counters(a, ts.done, ts.att);
}

// K1c: the same, FUSED over a range of iterations (single-GPU runs): one persistent launch in which every wave walks
// the schedule its[0..n_iters).  Saves the per-launch ramp, tail and RNG round trip.
//
// WORK POOLS.  Round 1 gave every wave a fixed quota per iteration and no grid barrier.  Free-running waves drift apart:
// one whose trips happen to be cheap runs iterations ahead of one whose trips are dear, so terms of several iterations —
// several values of eta — are applied side by side, and the last, finest iterations are finished by the stragglers alone.
// (The reference's iterations overlap by what its workers do in 1 ms, sgd.rs:366-403: a few per cent of an iteration.)
// Measured on the 525k-node bubble graph: relative error at path distance 1 of 0.195-0.246 depending on the stream count
// with free-running waves, 0.187-0.191 at every count with one launch per iteration — which is what the oracle's
// sequential mirror gives (profiles/r02/pacing.log).  A counting barrier per iteration (with a lag of 1-6 iterations)
// restores the precision but leaves the fast waves idle: C3 66-88 G updates/s against 93.
// Instead an iteration's min_term_updates updates are a POOL that the waves draw from in chunks of TEAM_CHUNK updates
// (one returning atomic per chunk, on one of up to 16 counters — one per 16 waves, sgd_kernel_common.h pool_slots — so that the
// claims do not queue on one address; a wave
// claims its next chunk before it works on the current one).  A wave moves on to iteration k + 1 when its counter of
// iteration k is exhausted: no wave is ever more than two chunks away from the others OF ITS COUNTER (the counters are fixed
// shares of an iteration: the waves of a fast one can run ahead of a slow one's — harmless for the sort, whose figures are the
// same with a launch per iteration; the layout kernel, K2c, uses one counter), nobody waits, and a wave that is
// slow simply takes fewer chunks — which is the reference's own rule (its workers share one count per iteration).  Every
// iteration still applies exactly min_term_updates updates with its own eta/theta.  C3: 97.8 G updates/s.
// (A single wave claims every chunk itself, in order: the kernel with fixed quotas works through its quota in the same
// chunks, so that one wave is bit for bit the oracle's mirror in both.)
// (POOL is a template parameter so that each build holds ONE inlined copy of the trip machine: with both launch modes in one
// kernel the pooled path spilled 65 VGPRs into 188 B of scratch per lane — and a first dispatch that needs more scratch than any
// kernel before it makes the runtime re-size the queue's scratch, the ~0.12 ms "first-dispatch latency" of profiles/r02/launch_gap.log.)
template <int B, bool LDS_TABLES, bool POOL>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) sgd1d_team_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters,
                                                                                   uint32_t *pool) {
    constexpr bool ATOMIC_LOADS = true;
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a0, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= a0.n_streams) return;
    const uint64_t T = a0.n_streams;
    KArgs a = a0;
    TeamState ts;
    ts.rng.s0 = a.rng[tid]; ts.rng.s1 = a.rng[T + tid]; ts.rng.s2 = a.rng[2 * T + tid]; ts.rng.s3 = a.rng[3 * T + tid];
    const int lane = threadIdx.x & 63;
    load_pass(a, tid, ts);
    if (POOL) {
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), n_waves = a0.n_streams >> 6;   // (scalar registers)
        const uint32_t slots = pool_slots(n_waves), slot = wave % slots;
        const uint64_t total = (uint64_t)a0.quota_base * a0.n_streams + a0.quota_rem;
        const uint32_t cap = (uint32_t)(total / slots + (slot < total % slots ? 1u : 0u));   // < 2^31 (host-checked)
        uint32_t k = 0, claim = 0;
        a.it = its[0];
        if (lane == 0) claim = __hip_atomic_fetch_add(pool + slot * POOL_STRIDE, a0.chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (k < n_iters) {
            const uint32_t old = (uint32_t)__builtin_amdgcn_readfirstlane((int)claim);
            if (old >= cap) {                                          // this iteration's pool is exhausted
                if (++k == n_iters) break;
                a.it = its[k];                                         // wave-uniform: scalar loads
                if (lane == 0) claim = __hip_atomic_fetch_add(pool + ((size_t)k * POOL_SLOTS + slot) * POOL_STRIDE, a0.chunk,
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                continue;
            }
            // the next claim travels while this chunk is worked on
            if (lane == 0) claim = __hip_atomic_fetch_add(pool + ((size_t)k * POOL_SLOTS + slot) * POOL_STRIDE, a0.chunk,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            team_iteration<B, LDS_TABLES, ATOMIC_LOADS, false>(a, path_tab, zeta_tab, ts, tid, cap - old < a0.chunk ? cap - old : a0.chunk, its + k);
        }
    } else {
        // fixed quota per wave and iteration, free-running (GFS_F_DBG_FREE_RUNNING)
        const uint64_t wq = wave_quota_of(a, tid);
        for (uint32_t k = 0; k < n_iters; ++k) {
            a.it = its[k];
            for (uint64_t done = 0; done < wq; done += a.chunk)
                team_iteration<B, LDS_TABLES, ATOMIC_LOADS, false>(a, path_tab, zeta_tab, ts, tid, wq - done < a.chunk ? wq - done : a.chunk, its + k);
        }
    }
    a.rng[tid] = ts.rng.s0; a.rng[T + tid] = ts.rng.s1; a.rng[2 * T + tid] = ts.rng.s2; a.rng[3 * T + tid] = ts.rng.s3;
    store_pass(a, tid, ts);
    flush_counters(a, ts.done, ts.att);
}

// ------------------------------------------------------------------------------------------
// Multi-GPU replica merge (no reference equivalent; gfasort_amd/distributed.py).  Two streaming
// kernels around the one all-reduce of an iteration:
//   prepare: buf[0][k] = (float)(x[k] - x_prev[k])  (this rank's batch),  buf[1][k] = delta != 0
//   apply  : x_prev[k] += sum_delta[k] / max(1, sum_touched[k]);  x[k] = x_prev[k]
// The exchanged buffer is f32 (half the xGMI bytes; a delta is rounded to 24 bits, 6e-8 relative,
// far below the SGD noise; all ranks apply the same reduced values, so replicas stay identical).
// Grid-stride, pure HBM streaming.
// ------------------------------------------------------------------------------------------
__global__ void merge_prepare_kernel(const double *x, const double *x_prev, float *buf, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 2;
    for (uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; k < n; k += stride) {
        if (k + 1 < n) {
            const double2 a = *reinterpret_cast<const double2 *>(x + k), b = *reinterpret_cast<const double2 *>(x_prev + k);
            const float d0 = (float)(a.x - b.x), d1 = (float)(a.y - b.y);
            *reinterpret_cast<float2 *>(buf + k) = make_float2(d0, d1);
            // the touched row starts at buf + n: 8-byte aligned only when n is even
            if (n & 1) { buf[n + k] = d0 != 0.f ? 1.f : 0.f; buf[n + k + 1] = d1 != 0.f ? 1.f : 0.f; }
            else *reinterpret_cast<float2 *>(buf + n + k) = make_float2(d0 != 0.f ? 1.f : 0.f, d1 != 0.f ? 1.f : 0.f);
        } else {
            const float d = (float)(x[k] - x_prev[k]);
            buf[k] = d; buf[n + k] = d != 0.f ? 1.f : 0.f;
        }
    }
}
__global__ void merge_apply_kernel(double *x, double *x_prev, const float *buf, uint64_t n, double scale_all) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const double c = (double)buf[n + k];
        const double div = scale_all > 0.0 ? scale_all : (c > 1.0 ? c : 1.0);
        const double v = x_prev[k] + (double)buf[k] / div;
        x_prev[k] = v; x[k] = v;
    }
}
hipError_t launch_merge_prepare(const double *x, const double *x_prev, float *buf, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(merge_prepare_kernel, dim3(2048), dim3(256), 0, st, x, x_prev, buf, n);
    return hipGetLastError();
}
hipError_t launch_merge_apply(double *x, double *x_prev, const float *buf, uint64_t n, double scale_all, hipStream_t st) {
    hipLaunchKernelGGL(merge_apply_kernel, dim3(2048), dim3(256), 0, st, x, x_prev, buf, n, scale_all);
    return hipGetLastError();
}

// Fused ranges of iterations: K1d for reference streams (pooled only); K1c only for the team kernel with its widest bundles (what
// the auto policy picks on graphs large enough for launch overhead to matter), pooled or with GFS_F_DBG_FREE_RUNNING's fixed quotas.
template <int B>
static const void *team_fused_kernel_1d(const KernelShape &s, bool pooled) {
    return with_flag(pooled, [&](auto P) { return with_flag(s.lds_tables, [&](auto L) { return kernel_addr(sgd1d_team_fused_kernel<B, L(), P()>); }); });
}
const void *fused_kernel_1d(const KernelShape &s, bool pooled) {
    switch (s.bundle) {
        case 16: return team_fused_kernel_1d<16>(s, pooled);
        case 32: return team_fused_kernel_1d<32>(s, pooled);
        case 64: return team_fused_kernel_1d<64>(s, pooled);
        case 0: case 1: return pooled ? with_flag(s.lds_tables, [](auto L) { return kernel_addr(sgd1d_fused_kernel<L()>); }) : nullptr;
        default: return nullptr;
    }
}
size_t pool_bytes(uint64_t n_iters) { return (size_t)n_iters * POOL_SLOTS * POOL_STRIDE * sizeof(uint32_t); }

// K1 for reference streams, K1b<B> for bundles of 4..64 (its debug trace always reads with agent-scope loads)
template <int B>
static const void *team_kernel_1d(const KernelShape &s) {
    return with_flag(s.lds_tables, [&](auto L) { return with_flag(s.atomic_loads, [&](auto A) { return with_flag(s.trace, [&](auto T) {
        return kernel_addr(sgd1d_team_kernel<B, L(), A() || T(), T()>);
    }); }); });
}
const void *iteration_kernel_1d(const KernelShape &s) {
    switch (s.bundle) {
        case 0: case 1:
            return with_flag(s.lds_tables, [&](auto L) { return with_flag(s.atomic_loads, [&](auto A) { return with_flag(s.trace, [&](auto T) {
                return kernel_addr(sgd1d_kernel<L(), A(), T()>);
            }); }); });
        case 4:  return team_kernel_1d<4>(s);
        case 8:  return team_kernel_1d<8>(s);
        case 16: return team_kernel_1d<16>(s);
        case 32: return team_kernel_1d<32>(s);
        case 64: return team_kernel_1d<64>(s);
        default: return nullptr;
    }
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_1d() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&merge_prepare_kernel));
}

}  // namespace gfs
