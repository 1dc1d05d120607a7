// launch_policy.h — what a context launches, decided from plain facts: how many streams, which sampling bundle and run length,
// whether a range of iterations is one fused launch, and the per-launch arithmetic that goes with it (an iteration's constants,
// the crowding onset, the width of the step index).  Host only and free of HIP — plain structures in, plain structures out, no
// global and no environment variable — so that it can be compiled into a program of its own and tested on a machine without a GPU
// (tests/test_launch_policy_host.py builds it under the address and undefined-behaviour sanitizers).
//
// The policy needs one fact from the device in the middle, the workgroups per CU of the chosen fused kernel, which makes it two
// phases: capi.hip calls shape_before_residency, resolves the kernels and asks the runtime, then calls shape_after_residency.
#pragma once
#include "../../include/gfasort_hip.h"
#include "sgd_limits.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace gfs {

struct GraphFacts {
    uint64_t n_nodes = 0, n_steps = 0, n_paths = 0;
    uint32_t max_path_steps = 0;
    bool valid_paths = false;                // some path has more than one step (sgd.rs:250-256)
    const uint32_t *path_counts = nullptr;   // steps per path, n_paths of them
};
struct DeviceFacts { int cu_count = 0; };

struct LaunchShape {
    // as asked (carried from phase one to phase two and to the kernel selection)
    int dims = 0;                      // 0 = 1D
    uint32_t flags = 0;
    bool trace = false, explicit_streams = false;
    // decided by shape_before_residency
    uint32_t block = 256;
    uint64_t n_streams = 0, quota_total = 0, attempt_factor = 0;
    uint32_t bundle = 1;               // lanes per sampling bundle actually used (1 = reference streams)
    uint32_t partners = 1;             // partner draws per leader (2: 1D team kernel at B = 64)
    uint32_t chain = 1;                // longest run in trips (sgd_device.h run_trips); 1 = a run is one trip
    // GFS_F_PHASED (K1e, sgd_kernels_1d_phased.hip): iterations [win_begin, win_end) run reference streams, the others the team
    // sampler at B = 64.  phased is false where the flag is a no-op (the auto policy picked another bundle).
    bool phased = false;
    uint64_t win_begin = 0, win_end = 0;
    bool lds_tables = true, atomic_loads = true;
    size_t lds_bytes = 0;
    uint64_t zlen_full = 0, zlen_staged = 0;
    bool team = false;                 // has_fused_team_kernel(dims, bundle): the only shapes whose residency is asked for
    // decided by shape_after_residency (which may also lower n_streams)
    uint64_t fused_resident_blocks = 0; // workgroups of the fused team kernel the chip holds at once (block size, LDS table)
    bool fused = false;                // a range of iterations is ONE launch; false: one launch per iteration
    bool pooled = false;               // ... of the kernel that draws from work pools (false: GFS_F_DBG_FREE_RUNNING's fixed quotas)
    bool fuse_one = false;             // a range of ONE iteration is a fused launch too, in chunks of one_chunk
    bool fuse_one_probe = false;       // ... or would be if GFS_DBG_ONE_CHUNK asked for it
    uint32_t one_chunk = 0;
    // decided by shape_records
    bool compact = false;              // the trips of K1b / K1c at B = 64 read the 8-byte trip records instead of the step records
};

// What the index build found in the step records it wrote (index_set_kernels.hip), and whether the 8-byte array stands beside them.
struct RecordFacts {
    uint64_t max_pos = 0;              // largest bp position of a step
    uint32_t max_a = 0, max_b = 0;     // largest crowding exponents of a step's node (sgd_device.h crowd_shift)
    bool have_trip_rec = false;        // trip_rec[s] = { slot, pos lo } was written and is still allocated
};

// "This context has a fused team kernel": K1c (K1e where phased) at the sort's widest bundles, K2c for layouts of 2 and more
// dimensions at B = 64.  Such a context is bounded by residency, keeps the schedule's constants resident and draws two partners
// per leader at B = 64 (choose_bundle).
inline bool has_fused_team_kernel(int dims, uint32_t bundle) { return (dims == 0 && bundle >= 16) || (dims >= 2 && bundle == 64); }

// The arguments of a setup that are refused whatever the graph is.
inline int check_setup_args(const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg, std::string *err) {
    if (!p) { *err = "params is null"; return GFS_E_ARG; }
    if (!(p->theta >= 0.0 && p->theta < 1.0)) { *err = "theta must be in [0,1)"; return GFS_E_ARG; }
    if (p->space_quantization_step == 0) { *err = "space_quantization_step must be > 0"; return GFS_E_ARG; }
    if (!(p->eta_max > 0.0)) { *err = "eta_max must be > 0"; return GFS_E_ARG; }
    if (dims < 0 || dims > GFS_MAX_DIMS) { *err = "dimensions must be 1..8"; return GFS_E_UNSUPPORTED; }
    if (cfg && (cfg->flags & GFS_F_PHASED)) {
        if (dims != 0) { *err = "GFS_F_PHASED is a sampler of the 1D sort: layouts have none"; return GFS_E_ARG; }
        const uint32_t b = (cfg->flags >> 16) & 0xFFu;
        if (b != 0 && b != 64) { *err = "GFS_F_PHASED switches between reference streams and bundles of 64: GFS_F_BUNDLE must be 0 or 64"; return GFS_E_ARG; }
    }
    return GFS_OK;
}

// Streams per launch when the caller leaves it to the library.
inline uint64_t auto_stream_count(const GraphFacts &g, const DeviceFacts &dev, int dims, uint64_t quota_total, bool team) {
    // Lanes per CU: each wave is a serial chain of memory round trips, so more chains raise throughput until the memory-side
    // atomic units saturate.  Round 1 (profiles/r01/sweep_streams_final.log, defer_probe.log): C3 69.1 / 78.7 / 80.2 G
    // updates/s at 512 / 768 / 976 lanes per CU, C4 layout flat from 768 up; reference streams flat within 5 % from 512 up.
    // Round 2: the 1D team kernels run 4 waves per SIMD (128 VGPRs; twin trips keep three blocks of a trip in flight) = 1024
    // lanes per CU; 5 waves (96 VGPRs) spill 58 registers and are slower (profiles/r02/two_partners.log).  The fused launch
    // further bounds the count by the workgroups that are resident at once (shape_after_residency).
    // The layout team kernels live on registers (a twin trip holds six records and three ends' coordinates): built for 3 waves
    // per SIMD (165 VGPRs at D = 2, nothing spilled) = 768 lanes per CU, for 2 from D = 3 up (176 at D = 3, 192-246 at D = 4..8)
    // = 512 (sgd_limits.h nd_waves_for; round 2's kernel needed 203 and ran two).
    const uint64_t chip = (uint64_t)dev.cu_count * ((team && dims == 0) ? 1024 : (team && dims >= 2) ? 256u * (unsigned)nd_team_waves(dims) : 976);
    // keep >= 8 updates per stream per batch on small graphs
    const uint64_t by_work = ((quota_total + 7) / 8 + 63) / 64 * 64;
    // and never more than one stream per 4 nodes (<= 0.5 in-flight terms per node): every in-flight
    // term corrects its two nodes from positions read before the others landed, so with ~2 concurrent
    // terms per node and mu clamped at 1 the corrections overshoot — a 6000-node graph of short paths
    // diverged (stress 1e8) under 6784 reference streams and converges under 1024
    // (profiles/r01/stream_cap_probe.log).  The team kernels tolerate three streams per 4 nodes: with the work pools of the
    // fused launch, bubble graphs of 26k / 79k / 197k nodes keep their relative error at path distance 1 (0.194 / 0.206 /
    // 0.192-0.197 against 0.198 / 0.208 / 0.191 at one stream per 2 nodes; reference streams 0.192 / 0.201 / 0.190) up to
    // one stream per node and lose it at two (0.224 / 0.248 / 0.220), at 2.0 / 1.65 / 1.2 times the rate
    // (profiles/r02/stream_cap_pools.log; round 1 allowed one per 2 nodes, measured with free-running waves whose drift
    // cost precision by itself).  An explicit n_streams overrides this.
    // Round 3 re-measured the bound (medium graphs leave the chip partly empty under it).  Bubble graphs of 66k / 131k / 302k
    // nodes keep every octave of the relative error within 4 % of reference streams up to 1.5 streams per node and lose distance
    // 1 at 2.0 (profiles/r03/stream_cap_probe.log) — but a window graph whose 16 paths each cover 5/8 of its 200k nodes loses its
    // exact chain order at 1.0 per node (3-115 inversions) and is scrambled at 1.25 (profiles/r03/chain_cap_probe.log), where
    // three per 4 nodes is exact on every graph tried.  The bound stays.
    const uint64_t by_nodes = (team ? g.n_nodes * 3 / 4 : g.n_nodes / 4) / 64 * 64;
    return std::max<uint64_t>(64, std::min(chip, std::min(by_work, by_nodes)));
}

// Sampling bundle: flags bits 16..23: 0 = auto, 1 = reference streams, 4..64 explicit (sgd_device.h).  Needs n_streams and
// quota_total; sets bundle, partners and chain.
inline int choose_bundle(const GraphFacts &g, int dims, uint32_t flags, LaunchShape *s, std::string *err) {
    uint32_t b = (flags >> 16) & 0xFFu;
    const bool b_auto = b == 0;
    if (b > 1 && (s->n_streams % 64 != 0 || (b != 4 && b != 8 && b != 16 && b != 32 && b != 64))) {
        *err = "bundled sampling needs n_streams % 64 == 0 and a bundle of 4, 8, 16, 32 or 64"; return GFS_E_ARG;
    }
    if (b > 1 && dims != 0 && b == 4) { *err = "bundled layout kernels exist for 1..8 dimensions and bundles of 8..64"; return GFS_E_UNSUPPORTED; }
    if (b == 0) {
        // auto (measured: profiles/r03/policy_sweep.log — bubble graphs of 16k...300k nodes, three seeds per cell, the relative
        // error per octave of path distance against reference streams): on graphs of >= 16 384 nodes the widest bundle for
        // which >= 95 % of the steps lie in paths of at least 4*B steps.  B = 64 with long runs is within 2-7 % of reference
        // streams in every octave from 16k nodes up and 2-10 times faster; narrower bundles and runs of one trip are both slower
        // and worse (+16...42 % at 64-127 steps from 131k nodes up: a run's two blocks move rigidly and leave a step at their edges,
        // short runs have more edges).  Round 2's extra condition — ">= 4096 independent leader draws per iteration" — is gone:
        // graphs with 37-99 leader draws per iteration are in that table and are as good as those with thousands; the run
        // length, not the number of leaders, is what the quality follows (bounded below by a floor of 64 leaders, see K).
        // Smaller graphs run reference streams: DRB1 (5k nodes) converged visibly slower with bundles (round 1).
        // Layouts of 4..8 dimensions keep reference streams: their team kernels (sgd_kernels_nd_team_wide.hip) are reached with an
        // explicit GFS_F_BUNDLE; whether auto should pick them rests on their rates and quality and is not decided here.
        b = 1;
        if (s->n_streams % 64 == 0 && dims <= 3 && g.n_nodes >= 16384) {
            for (uint32_t cand : {64u, 32u, 16u, 8u, 4u}) {
                if (cand == 4u && dims != 0) continue;
                uint64_t long_steps = 0;
                for (uint64_t p = 0; p < g.n_paths; ++p) if (g.path_counts[p] >= 4 * cand) long_steps += g.path_counts[p];
                if ((double)long_steps >= 0.95 * (double)g.n_steps) { b = cand; break; }
            }
        }
    }
    s->bundle = b;
    // Long runs (sgd_device.h run_trips): flags bits 24..31, 0 = auto.  Only the team kernels at B = 64 chain trips;
    // auto = 64 trips (runs of up to 4096 steps, adapted per path): the relative error of the layout, measured per octave
    // of path distance, is then within 10 % of reference streams on bubble graphs of 0.5M and 2M nodes — below it at
    // short distances — for the oracle's mirror and on the GPU (profiles/r02/quality_probe_long_runs.log).
    uint32_t k = (flags >> 24) & 0xFFu;
    if (k > 64 || (k & (k - 1))) { *err = "GFS_F_CHAIN: the run length in trips must be a power of two <= 64"; return GFS_E_ARG; }
    // (layout kernels: 16 — on C4 runs of 64 trips cost 13 % of the rate, 30.8 against 34.2-35.5 G updates/s, and the error
    // profile of the 2-D layout is already below reference streams' at 16: profiles/r02/quality_probe_layout_k.log)
    const bool k_auto = k == 0;
    if (k == 0) k = dims ? 16 : 64;
    // Two partners per leader (sgd_device.h Leader): the team kernels at B = 64 (1D; layouts of 2 and more dimensions), unless
    // GFS_F_ONE_PARTNER
    s->partners = (b == 64 && has_fused_team_kernel(dims, b) && !(flags & GFS_F_ONE_PARTNER)) ? 2u : 1u;
    // ... auto: and short enough that an iteration still draws >= 64 leaders (a leader stands for up to 64 * K * partners
    // terms): at 16k nodes runs of 32 trips left 37 leaders per iteration and +6 % at path distance 1, runs of 16 (74 leaders)
    // +1 %; from 32k nodes up 37 leaders were within 3 % (same table).  Binds only below ~500k steps.
    // (only where the library picked the bundle as well: an explicit GFS_F_BUNDLE(64) keeps 64 / 16)
    if (k_auto && b_auto && b == 64) while (k > 1 && s->quota_total / (64ull * k * s->partners) < 64) k >>= 1;
    s->chain = b == 64 ? k : 1;
    return GFS_OK;
}

// Phase one: everything up to, and including, which kernel shapes are wanted.  GFS_NOTHING_TO_DO (shape untouched) for a graph
// without nodes or without a path of more than one step; otherwise GFS_OK, or a GFS_E_* code with its message in *err.
inline int shape_before_residency(const GraphFacts &g, const DeviceFacts &dev, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg_in,
                                  LaunchShape *shape, std::string *err) {
    int rc = check_setup_args(p, dims, cfg_in, err);
    if (rc) return rc;
    if (g.n_nodes == 0 || !g.valid_paths) return GFS_NOTHING_TO_DO;
    const gfs_launch_config cfg = cfg_in ? *cfg_in : gfs_launch_config{};
    LaunchShape s;
    s.dims = dims; s.flags = cfg.flags; s.trace = cfg.trace_per_stream != 0; s.explicit_streams = cfg.n_streams != 0;

    // The zeta table of sgd.rs:311-331 on the device.  Only indices reachable from
    // jump <= min(space, max_path_steps-1) are ever read (sgd.rs:462-469): those are staged (and, where the table is computed
    // by the library, summed: set_state_plan.h zeta_clamped_space).
    s.zlen_full = gfs_zeta_table_len(p);
    if (s.zlen_full > 0xFFFFFFFFull) { *err = "zeta table too long"; return GFS_E_UNSUPPORTED; }
    const uint64_t maxjump = std::min<uint64_t>(p->space, g.max_path_steps ? g.max_path_steps - 1 : 0);
    const uint64_t last_idx = maxjump > p->space_max
                                  ? p->space_max + (maxjump - p->space_max) / p->space_quantization_step + 1
                                  : maxjump;
    s.zlen_staged = std::min<uint64_t>(last_idx + 1, s.zlen_full);

    s.quota_total = cfg.term_updates_per_iteration ? cfg.term_updates_per_iteration : p->min_term_updates;
    s.block = cfg.block_size ? cfg.block_size : 256;
    if (s.block % 64 || s.block > 1024) { *err = "block_size must be a multiple of 64, <= 1024"; return GFS_E_ARG; }
    s.n_streams = cfg.n_streams ? cfg.n_streams : auto_stream_count(g, dev, dims, s.quota_total, false);
    if (s.n_streams > 0x7FFFFFFFull) { *err = "n_streams too large"; return GFS_E_ARG; }
    if (s.quota_total / s.n_streams + 1 > 0xFFFFFFFFull) { *err = "per-stream quota exceeds 2^32"; return GFS_E_UNSUPPORTED; }
    s.attempt_factor = cfg.attempt_factor ? cfg.attempt_factor : 64;
    if (s.attempt_factor > 0xFFFFFFFFull) { *err = "attempt_factor too large"; return GFS_E_ARG; }
    rc = choose_bundle(g, dims, cfg.flags, &s, err);
    if (rc) return rc;
    if (!cfg.n_streams && s.bundle > 1) s.n_streams = auto_stream_count(g, dev, dims, s.quota_total, true);   // both counts are multiples of 64
    if (cfg.flags & GFS_F_PHASED) {
        // the phased sampler where the team sampler at B = 64 runs; where the policy picked reference streams every iteration is
        // theirs already (the window is the whole schedule, the run the default's), and other bundles have no phased kernel
        s.phased = s.bundle == 64;
        if (s.phased) gfs_phase_window(p, &s.win_begin, &s.win_end);
        else if (s.bundle == 1) { s.win_begin = 0; s.win_end = p->iter_max + 1; }
    }
    if (dims != 0 && s.bundle > 1 && s.block > 256) { *err = "the layout team kernels are built for workgroups of at most 256 lanes"; return GFS_E_ARG; }
    s.atomic_loads = !(cfg.flags & GFS_F_PLAIN_LOADS);
    const size_t lds = (size_t)g.n_paths * 16 + (size_t)s.zlen_staged * 8;      // path records (uint4) and the staged zeta table
    s.lds_tables = !(cfg.flags & GFS_F_NO_LDS_TABLES) && lds <= 48 * 1024;
    s.lds_bytes = s.lds_tables ? lds : 0;
    s.team = has_fused_team_kernel(dims, s.bundle);
    *shape = s;
    return GFS_OK;
}

// Phase two.  per_cu: the workgroups of the fused team kernel one CU holds at once with this block size and LDS table (looked at
// for team shapes only).  Bounds the automatic stream count by residency and decides what a range of iterations launches.
inline void shape_after_residency(int per_cu, const DeviceFacts &dev, LaunchShape *shape) {
    LaunchShape &s = *shape;
    const bool ref = s.bundle == 1;
    const bool free_running = (s.flags & GFS_F_DBG_FREE_RUNNING) != 0;
    s.fused_resident_blocks = 0;
    if (s.team) {
        // The fused launch has no grid barrier: a workgroup that does not fit on the chip beside the others would walk
        // its whole schedule, early large-eta iterations included, after they have finished theirs — on a 525k-node graph
        // 5 such waves of 4101 were enough to wreck the layout (relative error 64 at path distance 1:
        // profiles/r02/streams_5_waves.log).  So the fused team kernel (sort and layout alike) is only launched with every
        // workgroup resident: ask the runtime how many fit per CU with this block size and LDS table (33 KB of zeta table = 4
        // blocks of 256 per CU, not 5), bound the automatic stream count by it, and run one launch per iteration when a caller
        // asks for more streams.
        s.fused_resident_blocks = (uint64_t)std::max(per_cu, 0) * dev.cu_count;
        const uint64_t resident = s.fused_resident_blocks * s.block;
        if (!s.explicit_streams && s.n_streams > resident && resident >= 64) s.n_streams = resident;
    }
    // One persistent launch for a range where a fused kernel exists: the team kernels above and reference streams in any
    // dimension (K1d / K2d).  The waves of a fused launch draw an iteration's updates from a work pool (a share per counter
    // beyond 2^31 — 3e10 updates per iteration — cannot be pooled: one launch per iteration then, unless the diagnostic
    // GFS_F_DBG_FREE_RUNNING asks for round 1's fixed quotas).  The team kernel is only fused with every workgroup resident —
    // which assumes this context has the device to itself: concurrent streams or a second rank on the same device can delay a
    // workgroup, harmlessly under pools (a late wave finds the counters exhausted and leaves), not so with fixed quotas.
    const uint64_t n_waves = (s.n_streams + 63) / 64;
    // (layouts draw an iteration from ONE counter, sgd_nd_team.h K2c: the whole iteration must stay below 2^31)
    const bool pool_ok = n_waves <= 0xFFFFFFFFull &&
                         s.quota_total / (s.dims != 0 && s.bundle > 1 ? 1u : pool_slots((uint32_t)n_waves)) < (1ull << 31);
    const bool team_fusable = s.team && (s.phased ? pool_ok && !free_running : pool_ok || free_running) &&
                              (s.n_streams + s.block - 1) / s.block <= s.fused_resident_blocks;   // every workgroup resident
    s.pooled = pool_ok && !(free_running && s.bundle > 1);
    // (the free kernel is the team shapes' alone, and never the phased sampler's: K1e, K1d, K2d draw from pools only)
    s.fused = (team_fusable || (ref && pool_ok)) && s.atomic_loads && !s.trace && !(s.flags & GFS_F_NO_FUSE);
    // A range of ONE layout iteration is drawn from the pool too where it is at least four chunks per wave: with fixed quotas a layout
    // launch's waves finish as far apart as their leaders' costs are (C4: 2.33 ms per iteration against 2.21 pooled, 2.04 inside
    // a fused range).  Not with shorter chunks for smaller iterations: the layout pool is ONE counter, and it takes ~2e7 claims/s
    // comfortably and 4e7 not (C4 in chunks of 1024 / 512 / 256: 2.41 / 3.05 / 5.24 ms).  Not for the sort either: its launches of
    // one iteration are short (C3: 0.16 ms with fixed quotas, 0.15 pooled in chunks of 1024, 0.10 inside a fused range)
    // (profiles/r03/one_iteration_launch_probe.log, launch_overhead_probe.log).
    s.one_chunk = s.dims ? ND_TEAM_CHUNK : TEAM_CHUNK;
    s.fuse_one_probe = team_fusable && pool_ok;
    s.fuse_one = s.fuse_one_probe && s.dims != 0 && s.quota_total / n_waves >= 4ull * s.one_chunk;
}

// ---- per-launch arithmetic ------------------------------------------------------------------------------------------------
// GFS_F_PHASED: iteration k is one of the window's (K1's, reference streams)
inline bool in_window(const LaunchShape &s, uint64_t k) { return s.phased && k >= s.win_begin && k < s.win_end; }

inline IterConsts iter_consts(const gfs_sgd_params &p, const std::vector<double> &etas, const LaunchShape &s, uint64_t k) {
    IterConsts it;
    double fc = std::floor(p.cooling_start * (double)p.iter_max);          // sgd.rs:297
    uint64_t first_cooling = !(fc > 0.0) ? 0 : (fc >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)fc);
    bool cooling = k > first_cooling;                                      // sgd.rs:393-396
    double theta = cooling ? 0.001 : p.theta;
    it.eta = etas[k];
    it.cooling = cooling ? 1 : 0;
    it.zeta2theta = 1.0 + gfs_fast_precise_pow(0.5, theta);                // sgd.rs:471 (== :143 bound)
    double omt = 1.0 - theta;                                              // sgd.rs:133
    it.omt_e = h_sat_i32(omt); it.omt_fb = omt - (double)it.omt_e;
    double alpha = 1.0 / (1.0 - theta);                                    // sgd.rs:132
    it.alpha_e = h_sat_i32(alpha); it.alpha_fb = alpha - (double)it.alpha_e;
    it._pad = in_window(s, k) ? 1 : 0;                                     // K1e: a window iteration (the other kernels ignore it)
    return it;
}

// crowding onset (sgd_device.h crowd_shift): four times the concurrency of an average node
inline int32_t crowd_kshift(uint64_t n_steps, uint64_t n_streams) {
    const uint64_t per = n_steps / std::max<uint64_t>(2 * n_streams, 1);
    int lg = 0; while (lg < 63 && (per >> (lg + 1)) != 0) ++lg;            // floor(log2(max(per, 1)))
    return lg + 2;
}

// Record width of the trips (sgd_1d.h TripRec): 8-byte trip records where a trip reads nothing of the other 8 bytes of a step
// record.  A trip reads the slot, the position and the crowding exponents.  The high position word is zero on every step iff the
// largest position is below 2^32.  crowd_shift<true> is max(0, a_i - kshift, a_j - kshift, b_i, b_j) over a term's two records:
// zero for EVERY pair iff max_a <= kshift and max_b == 0.  The kernels that have a compact build are K1b and K1c at B = 64
// without a trace (K1e, the phased sampler, keeps full records); GFS_F_FULL_RECORDS forces full records.
inline bool compact_records(const LaunchShape &s, const RecordFacts &r, int32_t kshift) {
    const bool kernel = s.dims == 0 && s.bundle == 64 && !s.trace && !s.phased;
    const bool graph = r.have_trip_rec && r.max_pos < (1ull << 32) && (int64_t)r.max_a <= (int64_t)kshift && r.max_b == 0;
    return kernel && graph && !(s.flags & GFS_F_FULL_RECORDS);
}
// (after shape_after_residency: kshift follows the final stream count)
inline void shape_records(const RecordFacts &r, int32_t kshift, LaunchShape *shape) { shape->compact = compact_records(*shape, r, kshift); }

// the step index is drawn with 64-bit arithmetic (sgd_device.h sample_step)
inline bool wide_index(uint64_t n_steps, uint32_t flags) { return n_steps > 0xFFFFFFFFull || (flags & GFS_F_DBG_WIDE_INDEX); }

// "This context's plan is the pooled fused reference-stream kernel, with the schedule's constants resident, and it has work":
// what a batch (capi_batch.hip gfs_batch_create, gfs_batch_run) can take into its launch.
inline bool batch_eligible(const LaunchShape &s, bool trace, bool has_resident_schedule, bool idle) {
    return !idle && s.bundle == 1 && !s.phased && s.fused && s.pooled && !trace && has_resident_schedule;
}

}  // namespace gfs
