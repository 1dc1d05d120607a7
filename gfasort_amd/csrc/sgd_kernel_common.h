// sgd_kernel_common.h — shared pieces of the SGD batch kernels (gfx950 / CDNA4, wave64).
//
// K1  sgd1d_kernel : one launch = one SGD iteration of path_linear_sgd      (src/sgd.rs:442-584)
// K2  sgdnd_kernel : one launch = one iteration of path_linear_sgd_layout   (src/sgd.rs:988-1156)
//
// Execution model: one lane = one Xoshiro256+ stream = one reference worker thread
// (seed + stream id, sgd.rs:431-432).  A launch replaces the reference's checker thread
// (sgd.rs:366-407): eta / theta / cooling are launch constants and every stream performs
// exactly its quota of successful term updates, so the number of updates per iteration is
// min_term_updates, not wall-clock dependent.
//
// Memory: this is an HBM/fabric-bound gather/scatter, no MFMA.  Per update the kernel touches
// two 16-B step records (random), two (1D) position words read with agent-scope relaxed
// atomic loads, and two no-return f64 atomic adds (global_atomic_add_f64: gfx950 has the
// native instruction, so no CAS loop).  The zeta table and the per-path records are staged
// once per workgroup into LDS.  RNG state lives in registers for the whole launch and is
// loaded/stored coalesced (SoA) at entry/exit.
#pragma once
#include "sgd_device.h"
#include "sgd_limits.h"

namespace gfs {

struct TraceTerm { uint32_t i, j; double d; };

template <bool ATOMIC_LOADS>
__device__ __forceinline__ double load_pos(const double *p) {
    if (ATOMIC_LOADS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
__device__ __forceinline__ void add_pos(double *p, double v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Stage zeta/path tables into LDS (or return the global pointers).
template <bool LDS_TABLES>
__device__ __forceinline__ void stage_tables(const KArgs &a, unsigned char *smem,
                                             const uint4 *&path_tab, const double *&zeta_tab) {
    if (LDS_TABLES) {
        uint4 *lp = reinterpret_cast<uint4 *>(smem);
        double *lz = reinterpret_cast<double *>(smem + (size_t)a.n_paths * sizeof(uint4));
        for (uint32_t k = threadIdx.x; k < a.n_paths; k += blockDim.x) lp[k] = a.path_rec[k];
        for (uint32_t k = threadIdx.x; k < a.zlen_staged; k += blockDim.x) lz[k] = a.zetas[k];
        __syncthreads();
        path_tab = lp; zeta_tab = lz;
    } else {
        path_tab = a.path_rec; zeta_tab = a.zetas;
    }
}

// (COUNTER_SLOTS: sgd_limits.h)
__device__ __forceinline__ void flush_counters(const KArgs &a, uint32_t done, uint32_t att) {
    // wave64 butterfly, one atomic per wave
    unsigned long long d = done, t = att;
    for (int off = 32; off > 0; off >>= 1) {
        d += __shfl_xor(d, off, 64);
        t += __shfl_xor(t, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        // one 64-byte line per slot, waves spread over COUNTER_SLOTS lines: thousands of atomics on ONE
        // address serialise at the memory side and showed up as tens of microseconds at the end of every launch
        const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        unsigned long long *slot = a.counters + (size_t)(wave & (COUNTER_SLOTS - 1)) * 8;
        atomicAdd(slot, d);
        atomicAdd(slot + 1, t);
    }
}

// A stream's four RNG words, SoA [4][n_streams]: coalesced at entry and exit, in registers in between.
__device__ __forceinline__ void load_rng(const KArgs &a, uint32_t tid, Rng &rng) {
    const uint64_t T = a.n_streams;
    rng.s0 = a.rng[tid]; rng.s1 = a.rng[T + tid]; rng.s2 = a.rng[2 * T + tid]; rng.s3 = a.rng[3 * T + tid];
}
__device__ __forceinline__ void store_rng(const KArgs &a, uint32_t tid, const Rng &rng) {
    const uint64_t T = a.n_streams;
    a.rng[tid] = rng.s0; a.rng[T + tid] = rng.s1; a.rng[2 * T + tid] = rng.s2; a.rng[3 * T + tid] = rng.s3;
}

// One term of a traced stream (TRACE kernels; the trace holds trace_per_stream terms per stream).
__device__ __forceinline__ void record_trace(const KArgs &a, uint32_t tid, uint32_t &ntr, uint32_t i, uint32_t j, double d) {
    if (ntr < a.trace_per_stream) {
        TraceTerm *tt = reinterpret_cast<TraceTerm *>(a.trace) + (size_t)tid * a.trace_per_stream + ntr;
        tt->i = i; tt->j = j; tt->d = d;
        ++ntr;
    }
}

// A team wave's quota of an iteration: the sum of its 64 lanes' per-stream quotas.  wave_first: the wave's first stream, tid & ~63.
// (The layout kernels pass it through readfirstlane: the quota, and with it every loop variable of the trip machine, is then
// wave-uniform for the compiler too — scalar registers and scalar arithmetic instead of 64 copies.  The 1D kernels do not: with it
// K1b and the free-running K1c spill 2 to 6 scalar registers they do not spill without.)
__device__ __forceinline__ uint64_t wave_quota_of(const KArgs &a, const uint32_t wave_first) {
    uint64_t wq = (uint64_t)a.quota_base * 64u;
    if (wave_first < a.quota_rem) wq += (a.quota_rem - wave_first) < 64u ? (a.quota_rem - wave_first) : 64u;
    return wq;
}

// The quota's rank cut-off: of the lanes that hold a valid term, those whose rank is below what remains of the wave's quota
// act; wave_done advances by their number.  A chunk, and so an iteration, applies exactly its count of updates.
__device__ __forceinline__ bool quota_cut(bool valid, const int lane, const uint64_t wave_quota, uint64_t &wave_done) {
    const unsigned long long vmask = __ballot(valid);
    const uint64_t remaining = wave_quota - wave_done;
    const uint32_t nvalid = (uint32_t)__popcll(vmask);
    if (valid && nvalid > remaining) valid = (uint32_t)__popcll(vmask & ((1ull << lane) - 1ull)) < remaining;
    wave_done += nvalid < remaining ? nvalid : remaining;
    return valid;
}

// The step of a layout term (sgd.rs:1107-1142): r such that end i moves by -r * deltas[d] and end j by +r * deltas[d].
template <int D>
__device__ __forceinline__ double layout_step(double (&deltas)[D], const double mu, const double term_dist) {
    double mag_sq = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) mag_sq += deltas[d] * deltas[d];                        // :1107-1113
    if (mag_sq == 0.0) { deltas[0] = 1e-9; mag_sq = 1e-18; }                           // :1116-1119
    const double mag = sqrt(mag_sq);                                                   // :1121
    const double delta = mu * (mag - term_dist) / 2.0;                                 // :1125
    return delta / mag;                                                                // :1142
}

// The launch constants of the kernel, read afresh from the kernel-argument segment (every kernel here takes its KArgs first,
// by value: offset 0).  The team kernels' sampler calls this once per pass (~1000 trips): scalar loads, and the ~40 scalar
// registers of constants only the sampler needs are then free while the trips run — held through them they were spilled to
// vector lanes and read back inside the trip machine (74 / 61 spilled in K2b / K1c).  The empty asm hides the pointer's
// origin, or the loads would be hoisted and kept live like the by-value copy.
__device__ __forceinline__ void reload_kargs(KArgs &as) {
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    typedef const __attribute__((address_space(4))) uint32_t kword;
    kword *kw = (kword *)kp;
    uint32_t *dw = reinterpret_cast<uint32_t *>(&as);
    static_assert(sizeof(KArgs) % 4 == 0, "KArgs is copied by words");
#pragma unroll
    for (unsigned i = 0; i < sizeof(KArgs) / 4; ++i) dw[i] = kw[i];
}

template <int B>
__device__ __forceinline__ uint32_t bcast(uint32_t v, int leader_lane) {
    if (B == 64) return (uint32_t)__builtin_amdgcn_readlane((int)v, leader_lane);     // wave-uniform leader
    return (uint32_t)__shfl((int)v, leader_lane, 64);
}


template <int B>
__device__ __forceinline__ uint64_t bcast_first(const Leader &L, int leader_lane) {
    return ((uint64_t)bcast<B>(L.first_hi, leader_lane) << 32) | bcast<B>(L.first_lo, leader_lane);
}

// A team wave's pass across launches (KArgs.lead, [8][n_streams] SoA; State: TeamState, NdTeamState).
// lead word 5: ok bits of partner 0 (0..4) | the pass's end flips (5..7: layouts; 0 in the 1D sort) | trips left (8..15) |
// cooling (16) | colour (17) | seg (18..25) | partner (26) | ok bits of partner 1 (27..31)
template <class State>
__device__ __forceinline__ void load_pass(const KArgs &a, uint32_t tid, State &ts, uint32_t &flips) {
    if (!a.lead) return;
    const uint64_t T = a.n_streams;
    ts.L.first_lo = a.lead[tid]; ts.L.first_hi = a.lead[T + tid]; ts.L.cnt = a.lead[2 * T + tid];
    ts.L.ra0 = a.lead[3 * T + tid]; ts.L.rb0 = a.lead[4 * T + tid];
    const uint32_t w = a.lead[5 * T + tid];
    ts.L.ra1 = a.lead[6 * T + tid]; ts.L.rb1 = a.lead[7 * T + tid];
    ts.L.ok = (w & 0x1Fu) | ((w >> 27) << 8);
    flips = (w >> 5) & 7u;
    // (the place in the pass is the same for all 64 lanes of the wave: scalar registers)
    const uint32_t ws = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
    ts.left = (ws >> 8) & 0xFFu; ts.cool = (ws >> 16) & 1u; ts.colour = (ws >> 17) & 1u; ts.seg = (ws >> 18) & 0xFFu; ts.p = (ws >> 26) & 1u;
}
template <class State>
__device__ __forceinline__ void store_pass(const KArgs &a, uint32_t tid, const State &ts, const uint32_t flips) {
    if (!a.lead) return;
    const uint64_t T = a.n_streams;
    a.lead[tid] = ts.L.first_lo; a.lead[T + tid] = ts.L.first_hi; a.lead[2 * T + tid] = ts.L.cnt;
    a.lead[3 * T + tid] = ts.L.ra0; a.lead[4 * T + tid] = ts.L.rb0;
    a.lead[5 * T + tid] = (ts.L.ok & 0x1Fu) | ((flips & 7u) << 5) | (ts.left << 8) | (ts.cool << 16) | (ts.colour << 17) | (ts.seg << 18) |
                          (ts.p << 26) | (((ts.L.ok >> 8) & 0x1Fu) << 27);
    a.lead[6 * T + tid] = ts.L.ra1; a.lead[7 * T + tid] = ts.L.rb1;
}

// Short-jump trips of a 64-lane run (|jump| < 64).  Only the lanes of every other group of |jump| lanes act
// (node-disjoint rule), and the partner of an acting lane is the step of a resting lane |jump| places on: both
// sides of the trip touch the SAME lines.  Issued as two instructions they are two requests per line for half a
// wave of updates, one straight after the other on the same lines — measured, these trips were 9 % of the trips
// and 16 % of the time.  When the whole trip lies inside the path (no wrap, no mirrored jump) the +r of a term is
// therefore handed to the resting lane that sits on its node, and ONE instruction carries every add of the trip;
// only partners beyond the run's ends are added by a second, nearly empty one.  Returns the signed jump, or 0.
template <int B>
__device__ __forceinline__ int merged_trip_shift(uint32_t ok, uint32_t cnt, uint32_t ra0, uint32_t rb0, uint32_t off) {
    if (B != 64 || (ok & 3u) != 1u || cnt < 128u) return 0;
    const int64_t s = (int64_t)rb0 - (int64_t)ra0;
    if (s == 0 || s >= 64 || s <= -64) return 0;
    uint64_t base = (uint64_t)ra0 + (uint64_t)off;                                     // first step of this trip
    if (base >= cnt) base -= cnt;
    if (base + 64u > cnt) return 0;                                                    // the trip would wrap
    if (s > 0 ? base + 63u + (uint64_t)s > (uint64_t)cnt - 1u : (int64_t)base + s < 0) return 0;
    return (int)s;
}
// first step of the trip that merged_trip_shift accepted (rank in the path)
__device__ __forceinline__ uint32_t merged_trip_base(uint32_t cnt, uint32_t ra0, uint32_t off) {
    uint64_t base = (uint64_t)ra0 + (uint64_t)off;
    if (base >= cnt) base -= cnt;
    return (uint32_t)base;
}

// ------------------------------------------------------------------------------------------
// WORK POOLS of a fused launch (K1c / K2c / K1e: team waves; K1d / K2d: reference streams): one persistent launch in which every
// wave walks the schedule its[0..n_iters) and claims each iteration's updates in chunks from shared counters.
//
// Round 1 gave every wave a fixed quota per iteration and no grid barrier.  Free-running waves drift apart:
// one whose trips happen to be cheap runs iterations ahead of one whose trips are dear, so terms of several iterations —
// several values of eta — are applied side by side, and the last, finest iterations are finished by the stragglers alone.
// (The reference's iterations overlap by what its workers do in 1 ms, sgd.rs:366-403: a few per cent of an iteration.)
// Measured on the 525k-node bubble graph: relative error at path distance 1 of 0.195-0.246 depending on the stream count
// with free-running waves, 0.187-0.191 at every count with one launch per iteration — which is what the oracle's
// sequential mirror gives (profiles/r02/pacing.log).  A counting barrier per iteration (with a lag of 1-6 iterations)
// restores the precision but leaves the fast waves idle: C3 66-88 G updates/s against 93.
// Instead an iteration's min_term_updates updates are a POOL that the waves draw from in chunks (one returning atomic per
// chunk, on one of up to POOL_SLOTS counters, one 64-B line each, so that the claims do not queue on one address; a wave
// claims its next chunk before it works on the current one).  A wave moves on to iteration k + 1 when its counter of
// iteration k is exhausted: no wave is ever more than two chunks away from the others OF ITS COUNTER (the counters are fixed
// shares of an iteration: the waves of a fast one can run ahead of a slow one's — harmless for the sort, whose figures are the
// same with a launch per iteration; the layout kernel, K2c, uses one counter), nobody waits, and a wave that is
// slow simply takes fewer chunks — which is the reference's own rule (its workers share one count per iteration).  Every
// iteration still applies exactly min_term_updates updates with its own eta/theta.  C3: 97.8 G updates/s.
// (A single wave claims every chunk itself, in order: the kernels with fixed quotas work through their quota in the same
// chunks, so that one wave is bit for bit the oracle's mirror in both.)
// (POOL_SLOTS, POOL_STRIDE and pool_slots(), the counters in use: sgd_limits.h)

// A wave's counter and that counter's share of an iteration's updates (< 2^31, host-checked): equal shares, the first
// total % slots counters one more; or the whole iteration on counter 0 (pool_share_single: layouts, K2c).
struct PoolShare { uint32_t slot, cap; };
__device__ __forceinline__ PoolShare pool_share(const KArgs &a, const uint32_t wave, const uint32_t n_waves) {
    const uint32_t slots = pool_slots(n_waves), slot = wave % slots;
    const uint64_t total = (uint64_t)a.quota_base * a.n_streams + a.quota_rem;
    return {slot, (uint32_t)(total / slots + (slot < total % slots ? 1u : 0u))};
}
__device__ __forceinline__ PoolShare pool_share_single(const KArgs &a) {
    return {0u, (uint32_t)((uint64_t)a.quota_base * a.n_streams + a.quota_rem)};
}

// Lane 0 claims `chunk` updates from a counter; the old count arrives in its `claim`.
__device__ __forceinline__ void send_claim(uint32_t *pool_counter, const uint32_t chunk, uint32_t &claim) {
    if ((threadIdx.x & 63u) == 0) claim = __hip_atomic_fetch_add(pool_counter, chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The walk of one wave.  a.it holds the constants of the iteration worked on (wave-uniform: scalar loads); chunk_of() gives the
// size of a claim for the iteration just loaded into a.it, and is asked once per iteration: the claim a wave sends ahead is
// always for the iteration it works in.  body(k, m): m updates of iteration k, m = the claim, or what was left of the share
// (the last chunk of a counter is ragged: cap - old).  K1c and K1d / K2d call it; K2c (sgd_nd_team.h) and K1e
// (sgd_kernels_1d_phased.hip) write the same loop out over pool_share / send_claim: through the helper they spill registers.
// A change to the walk is a change to those two copies as well.
// (The first counter's address is 32-bit arithmetic, the later ones' 64-bit, as in the loops this replaced: with 64 bits
// throughout K2d at D = 7 spills 14 more registers.)
template <class ChunkOf, class Body>
__device__ __forceinline__ void pool_walk(KArgs &a, const IterConsts *its, const uint32_t n_iters, uint32_t *pool, const PoolShare ps,
                                          ChunkOf &&chunk_of, Body &&body) {
    uint32_t k = 0, claim = 0;
    a.it = its[0];
    uint32_t chunk = chunk_of();
    send_claim(pool + ps.slot * POOL_STRIDE, chunk, claim);
    while (k < n_iters) {
        const uint32_t old = (uint32_t)__builtin_amdgcn_readfirstlane((int)claim);
        if (old >= ps.cap) {                                                           // this iteration's pool is exhausted
            if (++k == n_iters) break;
            a.it = its[k];
            chunk = chunk_of();
            send_claim(pool + ((size_t)k * POOL_SLOTS + ps.slot) * POOL_STRIDE, chunk, claim);
            continue;
        }
        send_claim(pool + ((size_t)k * POOL_SLOTS + ps.slot) * POOL_STRIDE, chunk, claim);   // the next claim travels while this chunk is worked on
        body(k, ps.cap - old < chunk ? ps.cap - old : chunk);
    }
}

// K1d / K2d: REFERENCE STREAMS, a range of iterations in ONE persistent launch.  The reference's workers never stop at an
// iteration boundary — the checker thread switches eta / theta / cooling under them (sgd.rs:366-403) — and they share ONE
// count of term updates per iteration (sgd.rs:579-583).  One launch per iteration costs a small graph more than its
// updates do (DRB1: 35 059 updates in 0.1 ms, most of it launch ramp and tail).  Here every wave claims an iteration's
// updates from the pool in chunks of REF_CHUNK_PER_LANE per live lane; a chunk is dealt to the lanes — each an ordinary
// reference stream — in equal shares.  ONE stream claims every chunk itself, in order, and is bit for bit the
// per-iteration kernel and the oracle's single stream (tested).  (REF_CHUNK_PER_LANE: sgd_limits.h)

// run(share, max_attempts): the stream's loop for `share` successful updates (ref_run_1d / ref_run_nd)
template <class Run>
__device__ __forceinline__ void ref_pooled_walk(KArgs &a, const IterConsts *its, const uint32_t n_iters, uint32_t *pool,
                                                const uint32_t tid, Run &&run) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_first = tid & ~63u;                                            // < n_streams (caller)
    const uint32_t nl = a.n_streams - wave_first < 64u ? a.n_streams - wave_first : 64u;   // live lanes of this wave
    const uint32_t chunk = nl * a.ref_chunk;
    pool_walk(a, its, n_iters, pool, pool_share(a, tid >> 6, (a.n_streams + 63u) >> 6), [&]() __attribute__((always_inline)) { return chunk; },
              [&](const uint32_t, const uint32_t m) __attribute__((always_inline)) {
        const uint32_t share = lane < nl ? m / nl + (lane < m % nl ? 1u : 0u) : 0u;
        if (share) run(share, (uint64_t)a.attempt_factor * share + 64u);
    });
}

}  // namespace gfs
