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
        load_rng(a, tid, rng);
        const uint32_t quota = a.quota_base + (tid < a.quota_rem ? 1u : 0u);
        const uint64_t max_att64 = (uint64_t)a.attempt_factor * quota + 1024u;
        const uint64_t max_att = max_att64 > 0xFFFFFFFFull ? 0xFFFFFFFFull : max_att64;
        uint32_t ntr = TRACE ? a.trace_cnt[tid] : 0;
        ref_run_1d<LDS_TABLES, ATOMIC_LOADS, TRACE>(a, path_tab, zeta_tab, rng, quota, max_att, tid, done, att, ntr);
        store_rng(a, tid, rng);
        if (TRACE) a.trace_cnt[tid] = ntr;
    }
    flush_counters(a, done, att);
}

// K1d: the same streams, a range of iterations in one persistent launch with work pools (sgd_kernel_common.h
// ref_pooled_walk, pool_walk).  RNG state stays in registers for the whole schedule.
template <bool LDS_TABLES>
__global__ void sgd1d_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters, uint32_t *pool) {
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
        ref_run_1d<LDS_TABLES, true, false>(a, path_tab, zeta_tab, rng, share, max_att, tid, done, att, ntr);
    });
    if (live) store_rng(a, tid, rng);
    flush_counters(a, done, att);
}


// (4 waves per SIMD = 128 VGPRs: a twin trip keeps three blocks in flight and the next trip's records are on their way; built
// for 5 waves — 96 VGPRs — the kernel spills 58 registers and is slower: 88.5 against 91.5 G updates/s on C3 with round 1's
// launch, profiles/r02/two_partners.log.  Before the twin trips a fifth wave was worth +3 %.)
// (COMPACT, here and in K1c: the trips read the 8-byte trip records — sgd_1d.h TripRec; B = 64 without a trace)
template <int B, bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE, bool COMPACT = false>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) sgd1d_team_kernel(const KArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;       // n_streams % 64 == 0 (host-checked)
    if (tid >= a.n_streams) return;                                   // whole waves only
    TeamState ts;
    uint32_t no_flips = 0;                                            // (the sort has no end flips)
    load_rng(a, tid, ts.rng);
    ts.ntr = TRACE ? a.trace_cnt[tid] : 0;
    load_pass(a, tid, ts, no_flips);
    const uint64_t wq = wave_quota_of(a, tid & ~63u);                 // worked through in chunks, like a pool (K1c)
    for (uint64_t done = 0; done < wq; done += a.chunk)
        team_iteration<B, LDS_TABLES, ATOMIC_LOADS, TRACE, COMPACT>(a, path_tab, zeta_tab, ts, tid, wq - done < a.chunk ? wq - done : a.chunk);
    store_rng(a, tid, ts.rng);
    if (TRACE) a.trace_cnt[tid] = ts.ntr;
    store_pass(a, tid, ts, 0u);
    flush_counters(a, ts.done, ts.att);
}

// K1c: the same, FUSED over a range of iterations (single-GPU runs): one persistent launch in which every wave walks
// the schedule its[0..n_iters) and draws each iteration's updates from its work pool in chunks of TEAM_CHUNK (sgd_kernel_common.h
// pool_walk has the reasons and the rules).  Saves the per-launch ramp, tail and RNG round trip.
// (POOL is a template parameter so that each build holds ONE inlined copy of the trip machine: with both launch modes in one
// kernel the pooled path spilled 65 VGPRs into 188 B of scratch per lane — and a first dispatch that needs more scratch than any
// kernel before it makes the runtime re-size the queue's scratch, the ~0.12 ms "first-dispatch latency" of profiles/r02/launch_gap.log.)
template <int B, bool LDS_TABLES, bool POOL, bool COMPACT = false>
__global__ void __attribute__((amdgpu_waves_per_eu(4, 4))) sgd1d_team_fused_kernel(const KArgs a0, const IterConsts *its, const uint32_t n_iters,
                                                                                   uint32_t *pool) {
    constexpr bool ATOMIC_LOADS = true;
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 *path_tab; const double *zeta_tab;
    stage_tables<LDS_TABLES>(a0, smem, path_tab, zeta_tab);
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= a0.n_streams) return;
    KArgs a = a0;
    TeamState ts;
    uint32_t no_flips = 0;                                            // (the sort has no end flips)
    load_rng(a, tid, ts.rng);
    load_pass(a, tid, ts, no_flips);
    if (POOL) {
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // (scalar registers)
        pool_walk(a, its, n_iters, pool, pool_share(a0, wave, a0.n_streams >> 6), [&]() __attribute__((always_inline)) { return a0.chunk; },
                  [&](const uint32_t k, const uint32_t m) __attribute__((always_inline)) {
            team_iteration<B, LDS_TABLES, ATOMIC_LOADS, false, COMPACT>(a, path_tab, zeta_tab, ts, tid, m, its + k);
        });
    } else {
        // fixed quota per wave and iteration, free-running (GFS_F_DBG_FREE_RUNNING)
        const uint64_t wq = wave_quota_of(a, tid & ~63u);
        for (uint32_t k = 0; k < n_iters; ++k) {
            a.it = its[k];
            for (uint64_t done = 0; done < wq; done += a.chunk)
                team_iteration<B, LDS_TABLES, ATOMIC_LOADS, false, COMPACT>(a, path_tab, zeta_tab, ts, tid, wq - done < a.chunk ? wq - done : a.chunk, its + k);
        }
    }
    store_rng(a, tid, ts.rng);
    store_pass(a, tid, ts, 0u);
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
    if (s.compact) {
        if (s.bundle != 64) return nullptr;
        return with_flag(pooled, [&](auto P) { return with_flag(s.lds_tables, [&](auto L) { return kernel_addr(sgd1d_team_fused_kernel<64, L(), P(), true>); }); });
    }
    switch (s.bundle) {
        case 16: return team_fused_kernel_1d<16>(s, pooled);
        case 32: return team_fused_kernel_1d<32>(s, pooled);
        case 64: return team_fused_kernel_1d<64>(s, pooled);
        case 0: case 1: return pooled ? with_flag(s.lds_tables, [](auto L) { return kernel_addr(sgd1d_fused_kernel<L()>); }) : nullptr;
        default: return nullptr;
    }
}

// K1 for reference streams, K1b<B> for bundles of 4..64 (its debug trace always reads with agent-scope loads)
template <int B>
static const void *team_kernel_1d(const KernelShape &s) {
    return with_flag(s.lds_tables, [&](auto L) { return with_flag(s.atomic_loads, [&](auto A) { return with_flag(s.trace, [&](auto T) {
        return kernel_addr(sgd1d_team_kernel<B, L(), A() || T(), T()>);
    }); }); });
}
const void *iteration_kernel_1d(const KernelShape &s) {
    if (s.compact) {
        if (s.bundle != 64 || s.trace) return nullptr;
        return with_flag(s.lds_tables, [&](auto L) { return with_flag(s.atomic_loads, [&](auto A) { return kernel_addr(sgd1d_team_kernel<64, L(), A(), false, true>); }); });
    }
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
