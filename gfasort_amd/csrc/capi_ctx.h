// capi_ctx.h — what the units of the C ABI share and nobody else includes: the resident context (capi.hip) as the batch
// entries (capi_batch.hip) read it, error reporting, and the few functions of capi.hip that a batch calls (the owners of its
// memory and events: device_memory.h).  Nothing here is exported from the shared object.
#pragma once
#include "../../include/gfasort_hip.h"
#include "device_memory.h"
#include "sgd_kernel_common.h"
#include "launch_policy.h"
#include "sgd_host.h"
#include "readout_region.h"
#include "set_seed.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static inline int fail(int code, const std::string &msg) { return gfs_set_error(code, msg); }   // (the error slot: host_tables.hip)

// the records the diagnosis kernels write as words, and the read-outs' maps (readout_region.h) size by
static_assert(sizeof(gfs_path_error) == 8 * 8, "K7d / K7h write gfs_path_error as 8 words");
static_assert(sizeof(gfs_stretched_pair) == 5 * 8, "K7e / K7i write gfs_stretched_pair as 5 words");
static_assert(sizeof(gfs_node_error) == 3 * 8, "K7f / K7j write gfs_node_error as 3 words");

static constexpr size_t kCounterBytes = gfs::COUNTER_SLOTS * 8 * sizeof(unsigned long long);   // lines of 64 B

// The kernels of a configured context, resolved once by its setup (plan_setup) for the shape the policy decided (gfs_ctx::shape,
// launch_policy.h): everything of gfs_ctx_run_iteration / gfs_ctx_run_range that does not depend on the call.
struct LaunchPlan {
    const void *iteration = nullptr;         // K1 / K1b, K2 / K2b: one iteration per launch
    const void *window_iteration = nullptr;  // GFS_F_PHASED: K1, for the iterations of the window
    const void *fused = nullptr;             // K1c / K1d / K1e / K2c / K2d: a range of iterations per launch; null: one launch per iteration
    // the same two built for 8-byte trip records, where the shape has such a build (K1b / K1c at B = 64): launched instead of them
    // while gfs_ctx::shape.compact holds (launch_policy.h compact_records)
    const void *iteration_compact = nullptr, *fused_compact = nullptr;
};

struct gfs_ctx {
    int device = 0;
    int cu_count = 0;
    uint64_t n_nodes = 0, n_steps = 0, n_paths = 0;
    uint32_t max_path_steps = 0;
    bool valid_paths = false;
    bool set_item = false;             // owned by a gfs_ctx_set (capi_set.hip): its index arrays are borrowed from the set's arena, gfs_ctx_destroy leaves it alone
    std::vector<uint32_t> path_counts;
    std::vector<uint32_t> perm;        // dense node index (ABI order) -> internal index (device layout of positions)
    // device mirror of PathIndex: the five arrays lie in one arena — the context's own (gfs_ctx_create: a union of one item), or
    // its set's, and then this one stays empty — and borrow from it
    gfs::Buffer arena;                 // (declared before them: it outlives them)
    gfs::Array<uint4> d_step_rec;
    gfs::Array<uint2> d_trip_rec;      // { slot, pos lo } per step (+ the padding record), the context's own allocation, or null: written
                                       // by the index build where it could allocate it, kept while record_facts.max_pos < 2^32
    gfs::RecordFacts record_facts;     // what the index build found in the step records (launch_policy.h)
    gfs::Array<uint4> d_path_rec;
    gfs::Array<uint64_t> d_path_len;
    gfs::Array<uint32_t> d_perm;        // node layout on the device (dense index -> slot)
    gfs::Array<uint32_t> d_node_len;    // node lengths by dense index (K4: initial positions)
    // SGD state: every array but the positions lies in one arena and borrows from it — the context's own (gfs_ctx_setup_*: a set
    // setup of one item, freed by the next setup and by destroy), or its set's, and then this one stays empty.  The positions of a
    // context set up alone are an allocation of their own: they outlive a refused setup and go when a caller binds its own.
    gfs::Buffer state_arena;           // (declared before them: it outlives them)
    int dims = 0;                      // 0 = 1D
    bool configured = false;
    gfs_sgd_params params{};
    gfs_launch_config cfg{};
    std::vector<double> etas;
    gfs::Array<double> d_zetas;
    gfs::Array<double> d_x; uint64_t x_len = 0;               // (borrowed once a caller has bound its own: gfs_ctx_bind_positions)
    gfs::Array<uint64_t> d_rng;
    gfs::Array<uint32_t> d_lead;     // team kernels: the waves' partly expanded passes, [8][n_streams]
    gfs::Array<unsigned long long> d_counters;
    gfs::Array<gfs_term> d_trace; gfs::Array<uint32_t> d_trace_cnt;
    gfs::Array<gfs::SeedItem> d_seed_item; gfs::Array<uint32_t> d_seed_blocks;   // gfs_ctx_reset_streams: the tables of a seeding launch of this context alone
    gfs::Buffer d_its;                                        // schedule slice of a fused launch (arbitrary lists), grown on demand
    gfs::Array<gfs::IterConsts> d_its_all;                    // constants of iterations 0..=iter_max, resident
    gfs::Buffer d_pool;                // fused launch: per-iteration work pool counters (sgd_kernels_1d.hip), grown on demand
    gfs::LaunchShape shape;            // streams, bundle, run length, phase window, LDS tables, what a range launches (launch_policy.h)
    LaunchPlan plan;
    int32_t kshift_override = -1;      // test hook gfs_ctx_debug_kshift: >= 0 replaces the crowding onset of fill_kargs
    gfs::Buffer d_quality;             // K7 read-outs: scratch of 8-byte words, grown on demand and kept between calls and setups
    // timing
    std::vector<gfs::EventPair> events;
    size_t events_used = 0;
    double kernel_ms_harvested = 0.0;  // durations of event pairs already recycled
    uint64_t iterations = 0;
    uint64_t launches = 0;
    double total_ms = 0.0;
};

// What gfs_ctx_create checks of a graph view and derives from it on the host, shared with gfs_ctx_set_create (capi_set.hip), whose
// item i is what gfs_ctx_create gives: one statement of each check, `prefix` ("" or "set item <i>: ") in front of its text.
namespace gfs {
// the checks that read no array
static inline int check_view_counts(const gfs_graph_view *g, const std::string &prefix) {
    if (g->n_steps > (1ull << 40)) return fail(GFS_E_UNSUPPORTED, prefix + "more than 2^40 path steps");
    if (g->n_nodes > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, prefix + "more than 2^31-1 nodes");
    if (g->n_paths > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, prefix + "more than 2^31-1 paths");
    if (g->n_steps && (!g->step_node || !g->step_is_rev)) return fail(GFS_E_ARG, prefix + "null step arrays");
    if (!g->path_first_step) return fail(GFS_E_ARG, prefix + "null path_first_step");
    if (g->n_nodes && !g->node_len) return fail(GFS_E_ARG, prefix + "null node_len");
    return GFS_OK;
}
// ... and those that read path_first_step (step_node's range is checked on the device, in the pass that derives the node layout)
static inline int check_view_paths(const gfs_graph_view *g, const std::string &prefix) {
    if (g->path_first_step[0] != 0 || g->path_first_step[g->n_paths] != g->n_steps)
        return fail(GFS_E_ARG, prefix + "path_first_step must start at 0 and end at n_steps");
    for (uint64_t p = 0; p < g->n_paths; ++p)
        if (g->path_first_step[p + 1] < g->path_first_step[p]) return fail(GFS_E_ARG, prefix + "path_first_step not monotone");
    return GFS_OK;
}
// The facts the launch logic needs (path_counts, valid_paths, max_path_steps), and the two refusals made with them: a path of more
// than 2^32-1 steps, and — a step record keeps 55 bits of a step's bp position, its top bits carry the crowding exponents — a path
// of 2^55 bp or more, refused instead of truncated (cheap bound first, steps x longest node; the exact sum only where that fails).
static inline int path_facts(const gfs_graph_view *g, gfs_ctx *c, const std::string &prefix) {
    c->path_counts.reserve(g->n_paths);
    for (uint64_t p = 0; p < g->n_paths; ++p) {
        const uint64_t b = g->path_first_step[p], e = g->path_first_step[p + 1];
        if (e - b > 0xFFFFFFFFull) return fail(GFS_E_UNSUPPORTED, prefix + "a path with more than 2^32-1 steps");
        const uint32_t cnt = (uint32_t)(e - b);
        c->path_counts.push_back(cnt);
        if (cnt > 1) c->valid_paths = true;                               // sgd.rs:250-256
        if (cnt > c->max_path_steps) c->max_path_steps = cnt;
    }
    uint32_t max_len = 0;
    for (uint64_t k = 0; k < g->n_nodes; ++k) if (g->node_len[k] > max_len) max_len = g->node_len[k];
    for (uint64_t p = 0; p < g->n_paths; ++p) {
        const uint64_t b = g->path_first_step[p], e = g->path_first_step[p + 1];
        if ((unsigned __int128)(e - b) * max_len < ((unsigned __int128)1 << 55)) continue;
        unsigned __int128 bp = 0;
        for (uint64_t s = b; s < e; ++s) { const uint32_t n = g->step_node[s]; if (n < g->n_nodes) bp += g->node_len[n]; }
        if (bp >= ((unsigned __int128)1 << 55)) return fail(GFS_E_UNSUPPORTED, prefix + "a path of 2^55 bp or more");
    }
    return GFS_OK;
}
}  // namespace gfs

namespace gfs {
// GFS_TIMING: the phase times of an entry on stderr, each since the lap before it or (cumulative) since the start
struct Laps {
    const char *tag;
    bool cumulative;
    bool on = std::getenv("GFS_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, cumulative ? "[%s] %-10s %8.2f ms\n" : "[%s] %-12s %8.2f ms\n", tag, what,
                     std::chrono::duration<double, std::milli>(now - t).count());
        if (!cumulative) t = now;
    }
};

// capi_set.hip, for capi.hip: the ONE driver of the index build (K3b, index_set_kernels.hip), for a set's items and for a single
// context, which is a set of one.  ctxs[i] holds graphs[i]'s counts and path_facts; on GFS_OK its perm and its five index arrays
// are in place, the arrays borrowed from `arena`.  What tells a single context from a set's items, and nothing else:
//   arena      whose it is — the set's, or the single context's own (gfs_ctx::arena)
//   node_perm  a caller's layout (n == 1 only; checked to be a permutation by the caller, already in ctxs[0]->perm), or null
//   staged     a set: the inputs are gathered in ONE pinned staging copy, and the error texts say "set" and name the item;
//              else a single graph, which may be tens of GB: its arrays go up straight from the caller's, each with a blocking copy
// laps (nullable): GFS_TIMING of the caller's entry; the stream is drained before a lap where it is on.
// A single context also gets its 8-byte trip records and the facts of its records (gfs_ctx::d_trip_rec, record_facts) from the same
// pass; a set's items keep full records.
GFS_LOCAL int build_contexts(const gfs_graph_view *const *graphs, gfs_ctx *const *ctxs, uint64_t n, Buffer &arena, const uint32_t *node_perm,
                             bool staged, Laps *laps, gfs_ctx_set_info *info);
}  // namespace gfs

// capi.hip, for capi_set.hip: the host half of a setup, which the driver (setup_contexts, below) calls for every item.
namespace gfs {
// What a setup decides on the host before it touches its context: the launch shape and the kernels (launch_policy.h, the
// residency query in the middle), the eta schedule, the length of the position vector.  rc: GFS_OK, or GFS_NOTHING_TO_DO for a
// graph of 0 nodes (x_len 0) or without a path of more than one step (x_len set: it still gets its zeroed replica), and then
// shape, plan and etas are untouched.
struct SetupPlan {
    int rc = GFS_OK;
    int dims = 0;
    uint64_t x_len = 0;
    gfs_sgd_params params{};
    gfs_launch_config cfg{};
    LaunchShape shape;
    LaunchPlan plan;
    std::vector<double> etas;
};
// Reads c's facts, writes nothing of c.  p, dims and cfg have passed check_setup_args.  A refusal returns its code with its text
// in *err; out->x_len is set by then (a single context gets its zeroed replica whatever the policy says).
GFS_LOCAL int plan_setup(const gfs_ctx *c, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg, const double *etas,
                         SetupPlan *out, std::string *err);
// Bytes of state array `kind` (GFS_STATE_*) that a setup of this shape makes, 0 for one it does not: the sizes the state arena is
// planned with and gfs_ctx_debug_sgd_state reads.  has_work: the setup returned GFS_OK.
inline uint64_t state_bytes(uint32_t kind, bool has_work, uint64_t x_len, const LaunchShape &s, const gfs_sgd_params &p, const gfs_launch_config &cfg) {
    if (kind == GFS_STATE_POSITIONS) return x_len * 8;
    if (!has_work) return 0;
    const uint64_t T = s.n_streams;
    switch (kind) {
    case GFS_STATE_COUNTERS: return kCounterBytes;
    case GFS_STATE_LEAD: return s.bundle > 1 ? 8 * T * sizeof(uint32_t) : 0;          // team kernels, sort and layout
    case GFS_STATE_TRACE: return T * cfg.trace_per_stream * sizeof(gfs_term);
    case GFS_STATE_TRACE_COUNTS: return cfg.trace_per_stream ? T * sizeof(uint32_t) : 0;
    case GFS_STATE_RNG: return 4 * T * 8;
    case GFS_STATE_ZETAS: return s.zlen_full * 8;
    // the whole schedule's per-iteration constants, for fused launches over consecutive iterations
    case GFS_STATE_SCHEDULE: return (s.team || s.bundle == 1) && p.iter_max < (1u << 20) ? (p.iter_max + 1) * sizeof(IterConsts) : 0;
    default: return 0;
    }
}
inline uint64_t state_bytes(const SetupPlan &sp, uint32_t kind) { return state_bytes(kind, sp.rc == GFS_OK, sp.x_len, sp.shape, sp.params, sp.cfg); }
// the table of the whole schedule's constants (d_its_all), iterations 0..=iter_max, into out
GFS_LOCAL void schedule_table(const gfs_sgd_params &p, const std::vector<double> &etas, const LaunchShape &s, IterConsts *out);
// what a setup allocates or borrows, let go; the context is not set up afterwards
GFS_LOCAL void free_sgd_state(gfs_ctx *c);
// c's host fields from the plan, and the run's statistics back to zero; the state arrays are the caller's to put in place
GFS_LOCAL void commit_setup(gfs_ctx *c, SetupPlan &&sp);

// capi_set.hip, for capi.hip: the ONE driver of a setup (K3c), for a set's items and for a single context, which is a set of one.
// Every ctxs[i] set up as gfs_ctx_setup_1d / _nd would (dims[i] = 0 / 1..8; < 0: refused, "dimensions must be 1..8"): its state
// arrays laid out in `arena` by gfs_ctx_set_state_plan and borrowed from it, the seeding tables behind them; one memset, one copy,
// one seeding launch.  item_rc[i] (nullable): GFS_OK or GFS_NOTHING_TO_DO.  What tells a single context from a set's items, and
// nothing else:
//   arena     whose it is — the set's, kept across setups and regrown where too small, or the single context's own
//             (gfs_ctx::state_arena), which free_sgd_state releases at every setup
//   pinned    a set: its pinned staging, kept like the arena, which mirrors the uploaded range; the error texts name the item
//             ("set item <i>: "), a refusal names the lowest and leaves EVERY item as it was, and the positions lie in the arena.
//             null: a single context (n == 1).  Its range is staged in pageable memory (no hipHostMalloc per setup) and goes up in
//             one blocking copy; its positions are an allocation of its own (gfs_ctx::state_arena says why); and its refusals keep
//             their order: the arguments are checked before the context is touched, then it is let go (free_sgd_state; a layout
//             gives its trip records back), planned, committed and given its zeroed replica, and only then is a refusal of the
//             launch policy returned — the context not set up, the replica kept.
//   etas      a caller's schedule, iter_max + 1 doubles, into the plan (single only; null: computed)
//   zetas     a caller's zeta table, zlen_full doubles, in the place of the zeta slice in what goes up (single only; null: computed)
//   info      (nullable) what the call allocated, copied and launched: a set keeps it for gfs_ctx_set_get_setup_info
GFS_LOCAL int setup_contexts(gfs_ctx *const *ctxs, const gfs_sgd_params *const *params, const int *dims, const gfs_launch_config *cfgs,
                             uint64_t n, Buffer &arena, Buffer *pinned, const double *etas, const double *zetas, int32_t *item_rc,
                             gfs_ctx_set_setup_info *info);
}  // namespace gfs

// capi.hip, for capi_batch.hip
namespace gfs {
GFS_LOCAL void fill_kargs(const gfs_ctx *c, KArgs &a);
GFS_LOCAL IterConsts iter_consts(const gfs_ctx *c, uint64_t k);
GFS_LOCAL int check_step_distances(const uint64_t *zs, uint64_t n_z, const gfs_pair_error *out);
GFS_LOCAL int check_diagnosis(uint64_t z, double ratio);   // K7d-f and K7h-j: z >= 1, ratio a number >= 0
// five words of K7a / K7g { pairs, sum_rel_sq, max_rel_sq, sum_abs, sum_sq (f64 bits) } as the ABI's record for step distance z
GFS_LOCAL gfs_pair_error unpack_pair_error(uint64_t z, const uint64_t *w);
// five words of K7c / K7k { steps, abs_err_sum, genomic_sum, sq_err_sum (f64 bits), 0 } as the ABI's record; and the refusal of a
// graph whose length in bp a double no longer holds exactly, "batch item <i>: " in front of its text where batch_item >= 0
GFS_LOCAL gfs_sort_quality unpack_sort_quality(const uint64_t *w);
GFS_LOCAL int check_sorted_length(uint64_t total_bp, int64_t batch_item = -1);
}  // namespace gfs
