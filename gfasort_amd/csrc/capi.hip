// capi.hip — the device plumbing of the C ABI of libgfasort_hip.so (include/gfasort_hip.h): the resident
// context (device mirror of PathIndex + positions + RNG streams), its launches and read-outs, and the one-shot entry
// points that stand where path_linear_sgd / path_linear_sgd_layout stand in the reference.  What a context launches is decided in
// launch_policy.h; the host tables are host_tables.hip's; batches of contexts are capi_batch.hip's (capi_ctx.h is what the two share).
#include "capi_ctx.h"
#include "index_set.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>

extern "C" {

const char *gfs_version(void) { return "gfasort_hip 0.1.0 (gfx950)"; }
int gfs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int gfs_warmup(int device) {
    // Creates the HIP context (the first HIP call of a process costs ~0.1-0.3 s); callers run this
    // on a side thread while they are still parsing their input.
    gfs::Laps laps{"gfs_warmup", false};
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(GFS_E_HIP, "no HIP device available (libgfasort_hip has no CPU fallback)");
    if (device < 0 || device >= n) return fail(GFS_E_ARG, "bad device index");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(nullptr));
    laps.lap("context");
    // code objects load on first use, one per translation unit: touch each now, and the allocator too
    HIPCHK(gfs::warm_module_1d());
    HIPCHK(gfs::warm_module_1d_phased());
    laps.lap("module 1d");
    HIPCHK(gfs::warm_module_index());
    HIPCHK(gfs::warm_module_index_set());
    HIPCHK(gfs::warm_module_set_setup());
    HIPCHK(gfs::warm_module_quality());
    laps.lap("module index");
    HIPCHK(gfs::warm_module_nd());
    HIPCHK(gfs::warm_module_nd_team());
    HIPCHK(gfs::warm_module_nd_team_wide());
    laps.lap("modules nd");
    // ... and the copy paths in both directions (the first hipMemcpy of a process sets up its staging
    // buffers and DMA queues: ~0.13 s when it was left to the first upload)
    gfs::Buffer p;
    std::vector<unsigned char> h(1 << 20, 0);
    if (int rc = p.reserve(64u << 20)) return rc;
    laps.lap("malloc");
    HIPCHK(hipMemcpy(p.p, h.data(), h.size(), hipMemcpyHostToDevice));
    laps.lap("h2d");
    HIPCHK(hipMemset(p.p, 0, 64u << 20));
    HIPCHK(hipDeviceSynchronize());
    laps.lap("memset");
    HIPCHK(hipMemcpy(h.data(), p.p, h.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipDeviceSynchronize());
    laps.lap("d2h");
    p.reset();
    laps.lap("free");
    return GFS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// resident context
// ---------------------------------------------------------------------------------------------
// what a setup allocates, let go before the next one (the index of gfs_ctx_create and the read-outs' scratch stay)
void gfs::free_sgd_state(gfs_ctx *c) {
    c->d_zetas.reset();
    c->d_x.reset();                                                       // (a bound pointer is the caller's: only dropped)
    c->d_rng.reset();
    c->d_lead.reset();
    c->d_counters.reset();
    c->d_trace.reset();
    c->d_trace_cnt.reset();
    c->d_its.reset();
    c->d_its_all.reset();
    c->d_pool.reset();
    c->d_seed_item.reset();
    c->d_seed_blocks.reset();
    c->state_arena.reset();                                               // (after the arrays that borrowed from it)
    c->configured = false;
}

gfs::IterConsts gfs::iter_consts(const gfs_ctx *c, uint64_t k) { return gfs::iter_consts(c->params, c->etas, c->shape, k); }

// The resident table of the whole schedule's constants (d_its_all); again whenever the phase window moves, whose marks it carries.
void gfs::schedule_table(const gfs_sgd_params &p, const std::vector<double> &etas, const gfs::LaunchShape &s, gfs::IterConsts *out) {
    for (uint64_t k = 0; k <= p.iter_max; ++k) out[k] = gfs::iter_consts(p, etas, s, k);
}
static int upload_schedule(gfs_ctx *c) {
    std::vector<gfs::IterConsts> all(c->params.iter_max + 1);
    gfs::schedule_table(c->params, c->etas, c->shape, all.data());
    HIPCHK(hipMemcpy(c->d_its_all, all.data(), all.size() * sizeof(gfs::IterConsts), hipMemcpyHostToDevice));
    return GFS_OK;
}

// ---- kernels: one selection, one residency query, one launch -------------------------------------------------------------
// The dispatch over the kernel units (sgd_host.h): reference streams, the team kernels of D = 1..3 and those of D = 4..8.
static const void *iteration_kernel(const gfs::KernelShape &s) {
    if (s.dims == 0) return gfs::iteration_kernel_1d(s);
    if (s.bundle <= 1) return gfs::iteration_kernel_nd(s);
    return s.dims <= 3 ? gfs::iteration_kernel_nd_team(s) : gfs::iteration_kernel_nd_team_wide(s);
}
static const void *fused_kernel(const gfs::KernelShape &s, bool pooled) {
    if (s.dims == 0) return gfs::fused_kernel_1d(s, pooled);
    if (s.bundle <= 1) return gfs::fused_kernel_nd(s, pooled);
    return s.dims <= 3 ? gfs::fused_kernel_nd_team(s, pooled) : gfs::fused_kernel_nd_team_wide(s, pooled);
}
// Workgroups of `fn` one CU holds at once with this context's block size and LDS table (registers, waves per SIMD and the table
// all count).  Also: the first launch of a kernel function costs the host ~0.1 ms (the runtime materialises the function
// lazily), and a caller that brackets its launch with events pays that inside the bracket; this resolves the function at setup.
static int resident_blocks_per_cu(const gfs::LaunchShape &s, const void *fn, int *per_cu, std::string *err) {
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, fn);
    if (e != hipSuccess) { *err = std::string("hipFuncGetAttributes(&attr, fn): ") + hipGetErrorString(e); return GFS_E_HIP; }
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, (int)s.block, s.lds_bytes);
    if (e != hipSuccess) { *err = std::string("hipOccupancyMaxActiveBlocksPerMultiprocessor: ") + hipGetErrorString(e); return GFS_E_HIP; }
    return GFS_OK;
}

// Every kernel here takes its KArgs first, by value; the fused ones then (const IterConsts *its, uint32_t n_iters, uint32_t *pool).
static hipError_t launch(const gfs_ctx *c, const void *fn, gfs::KArgs &a, const gfs::IterConsts *its, uint32_t n_iters, uint32_t *pool,
                         hipStream_t st) {
    void *args[] = {&a, &its, &n_iters, &pool};                            // (a per-iteration kernel reads args[0] only)
    const gfs::LaunchShape &s = c->shape;
    const dim3 block(s.block), grid((unsigned)((s.n_streams + s.block - 1) / s.block));
    return hipLaunchKernel(fn, grid, block, args, s.lds_bytes, st);
}

// Resolves the plan for the shape as shape_before_residency left it, asks the runtime for the fused team kernel's residency and
// lets shape_after_residency finish the shape (which may lower n_streams).
// Then the record width (shape_records: the crowding onset follows the final stream count) and, where the kernels have one, the
// builds for 8-byte trip records.
static int plan_launches(int cu_count, const gfs::RecordFacts &rec, int32_t kshift_override, uint64_t n_steps, gfs::LaunchShape &s, LaunchPlan &pl,
                         std::string *err) {
    pl = LaunchPlan{};
    const gfs::KernelShape shape{s.dims, s.bundle, s.lds_tables, s.atomic_loads, s.trace};
    const bool team = s.team, ref = s.bundle == 1;
    const bool free_running = (s.flags & GFS_F_DBG_FREE_RUNNING) != 0;
    pl.iteration = iteration_kernel(shape);
    if (s.phased) pl.window_iteration = iteration_kernel({0, 1, s.lds_tables, s.atomic_loads, s.trace});
    const void *pooled_kernel = s.phased ? gfs::phased_fused_kernel(s.lds_tables) : (team || ref) ? fused_kernel(shape, true) : nullptr;
    const void *free_kernel = team && !s.phased && free_running ? fused_kernel(shape, false) : nullptr;   // (K1e, K1d, K2d: pools only)
    if (!pl.iteration || (s.phased && !pl.window_iteration) || ((team || ref) && !pooled_kernel) ||
        (team && !s.phased && free_running && !free_kernel)) {
        *err = "no kernel is built for dims=" + std::to_string(s.dims) + " bundle=" + std::to_string(s.bundle) +
               " lds_tables=" + std::to_string(s.lds_tables) + " atomic_loads=" + std::to_string(s.atomic_loads) +
               " trace=" + std::to_string(s.trace) + " phased=" + std::to_string(s.phased);
        return GFS_E_UNSUPPORTED;
    }
    // The builds for 8-byte trip records, where this shape has them (what compact_records asks of the kernel is decided by now;
    // what it asks of the graph waits for the final stream count).  A context may launch either width over its life
    // (gfs_ctx_debug_kshift moves the onset), so both are resolved here, and the residency is what both can hold.
    gfs::LaunchShape probe = s;
    probe.flags &= ~GFS_F_FULL_RECORDS;
    const bool has_compact = rec.have_trip_rec && gfs::compact_records(probe, gfs::RecordFacts{0, 0, 0, true}, 0);
    const gfs::KernelShape compact{s.dims, s.bundle, s.lds_tables, s.atomic_loads, s.trace, true};
    const void *pooled_compact = has_compact ? fused_kernel(compact, true) : nullptr;
    const void *free_compact = has_compact && free_running ? fused_kernel(compact, false) : nullptr;
    if (has_compact) pl.iteration_compact = iteration_kernel(compact);
    if (has_compact && (!pl.iteration_compact || !pooled_compact || (free_running && !free_compact))) {
        *err = "no kernel is built for 8-byte trip records in this shape"; return GFS_E_UNSUPPORTED;
    }
    int per_cu = 0;
    if (team) {                                                            // (the measurement behind it: shape_after_residency)
        int rc = resident_blocks_per_cu(s, pooled_kernel, &per_cu, err);
        if (rc) return rc;
        if (has_compact) {
            int per_cu_compact = 0;
            if ((rc = resident_blocks_per_cu(s, pooled_compact, &per_cu_compact, err))) return rc;
            per_cu = std::min(per_cu, per_cu_compact);
        }
    }
    gfs::shape_after_residency(per_cu, gfs::DeviceFacts{cu_count}, &s);
    if (s.fused) pl.fused = s.pooled ? pooled_kernel : free_kernel;
    if (s.fused && has_compact) pl.fused_compact = s.pooled ? pooled_compact : free_compact;
    gfs::shape_records(rec, kshift_override >= 0 ? kshift_override : gfs::crowd_kshift(n_steps, s.n_streams), &s);
    return GFS_OK;
}

// ---- a setup's host half (capi_ctx.h: shared with gfs_ctx_set_setup_*, capi_set.hip) -------------------------------------------
int gfs::plan_setup(const gfs_ctx *c, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg, const double *etas,
                    gfs::SetupPlan *out, std::string *err) {
    gfs::SetupPlan &sp = *out;
    sp = gfs::SetupPlan{};
    sp.params = *p;
    sp.cfg = cfg ? *cfg : gfs_launch_config{};
    sp.dims = dims;
    sp.rc = GFS_NOTHING_TO_DO;
    if (c->n_nodes == 0) return sp.rc;
    // positions.  A context with nothing to do (no path of more than one step: sgd.rs:250-261 returns before any
    // update) still owns a full-length position replica: a multi-GPU rank whose shard holds no such path must be able to
    // upload, bind, merge and download like its peers — its contribution to every merge is a zero delta of the same size.
    sp.x_len = dims ? c->n_nodes * 2 * (uint64_t)dims : c->n_nodes;
    if (!c->valid_paths) return sp.rc;

    // launch shape (launch_policy.h): decided before anything of the run's state is allocated
    const gfs::GraphFacts graph{c->n_nodes, c->n_steps, c->n_paths, c->max_path_steps, c->valid_paths, c->path_counts.data()};
    int rc = gfs::shape_before_residency(graph, gfs::DeviceFacts{c->cu_count}, p, dims, cfg, &sp.shape, err);
    if (rc) return rc;
    rc = plan_launches(c->cu_count, c->record_facts, c->kshift_override, c->n_steps, sp.shape, sp.plan, err);   // (may lower n_streams)
    if (rc) return rc;
    // eta schedule (host, bit-exact) unless supplied
    sp.etas.resize(p->iter_max + 1);
    if (etas) std::copy(etas, etas + p->iter_max + 1, sp.etas.begin());
    else gfs_sgd_schedule(p, sp.etas.data());
    return sp.rc = GFS_OK;
}

void gfs::commit_setup(gfs_ctx *c, gfs::SetupPlan &&sp) {
    const bool has_work = sp.rc == GFS_OK;
    c->params = sp.params; c->cfg = sp.cfg; c->dims = sp.dims; c->x_len = sp.x_len;
    c->shape = has_work ? sp.shape : gfs::LaunchShape{};
    c->plan = has_work ? sp.plan : LaunchPlan{};
    if (!has_work) return;
    c->etas = std::move(sp.etas);
    c->events_used = 0; c->kernel_ms_harvested = 0.0; c->iterations = 0; c->total_ms = 0.0;
}

// A single context's setup: a set setup of one item (capi_set.hip setup_contexts; capi_ctx.h says what is its own)
static int setup_common(gfs_ctx *c, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg,
                        const double *etas, const double *zetas) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    int32_t rc = GFS_OK;                                                   // GFS_OK or GFS_NOTHING_TO_DO
    const int bad = gfs::setup_contexts(&c, &p, &dims, cfg, 1, c->state_arena, nullptr, etas, zetas, &rc, nullptr);
    return bad ? bad : rc;
}

extern "C" {

int gfs_ctx_create(const gfs_graph_view *g, int device, gfs_ctx **out) {
    return gfs_ctx_create_with_layout(g, device, nullptr, out);
}

int gfs_ctx_create_with_layout(const gfs_graph_view *g, int device, const uint32_t *node_perm, gfs_ctx **out) {
    if (!g || !out) return fail(GFS_E_ARG, "null argument");
    *out = nullptr;
    if (int bad = gfs::check_view_counts(g, "")) return bad;               // (capi_ctx.h: shared with gfs_ctx_set_create)
    if (int bad = gfs::check_view_paths(g, "")) return bad;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GFS_E_HIP, "no HIP device available (libgfasort_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFS_E_ARG, "bad device index");
    gfs::Laps laps{"gfs_ctx_create", false};
    laps.lap("validate");
    // (every error return below relies on scope: the temporaries go first, then the context)
    std::unique_ptr<gfs_ctx, decltype(&gfs_ctx_destroy)> owner(new (std::nothrow) gfs_ctx(), gfs_ctx_destroy);
    gfs_ctx *c = owner.get();
    if (!c) return fail(GFS_E_NOMEM, "out of memory");
    c->device = device;
    c->n_nodes = g->n_nodes; c->n_steps = g->n_steps; c->n_paths = g->n_paths;
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(GFS_E_HIP, "hipGetDeviceProperties failed");
    c->cu_count = prop.multiProcessorCount;

    // Internal node layout.  The position vector is stored in FIRST-VISIT PATH ORDER (nodes in the
    // order the paths first step on them, unvisited nodes last; derived on the device, index_set_kernels.hip)
    // unless the caller supplies a layout: consecutive steps of a path then touch neighbouring position words whatever the
    // order of the input's S lines was, which is what lets a run's loads and atomics coalesce
    // (C3 with randomly ordered nodes: 63 G updates/s in path order, 11 G/s in input order).
    c->perm.assign(g->n_nodes, 0xFFFFFFFFu);
    if (node_perm) {
        std::vector<uint8_t> seen(g->n_nodes, 0);
        for (uint64_t k = 0; k < g->n_nodes; ++k) {
            if (node_perm[k] >= g->n_nodes || seen[node_perm[k]]) return fail(GFS_E_ARG, "node_perm is not a permutation");
            seen[node_perm[k]] = 1; c->perm[k] = node_perm[k];
        }
    }
    // The facts the launch logic needs, with the refusals of over-long paths (capi_ctx.h)
    if (int bad = gfs::path_facts(g, c, "")) return bad;
    // The index on the device (K3b, index_set_kernels.hip), as a union of one item in an arena of the context's own: the range
    // check of step_node, the layout unless given, and K3 — PathIndex::from_graph (sgd.rs:34-71), the per-path exclusive prefix
    // sum of node lengths over the steps, written straight into the 16-byte step records.  Uploads 5 B per step instead of 16.
    gfs_ctx_set_info info{};
    if (int bad = gfs::build_contexts(&g, &c, 1, c->arena, node_perm, false, &laps, &info)) return bad;
    laps.lap("free tmp");
    *out = owner.release();
    return GFS_OK;
}

void gfs_ctx_destroy(gfs_ctx *c) {
    if (!c || c->set_item) return;                                         // (a set's item goes with its set: gfs_ctx_set_destroy)
    (void)hipSetDevice(c->device);
    delete c;                                                              // (its buffers and events go here: the device is set)
}

int gfs_ctx_setup_1d(gfs_ctx *c, const gfs_sgd_params *p, const gfs_launch_config *cfg,
                     const double *etas, const double *zetas) {
    return setup_common(c, p, 0, cfg, etas, zetas);
}
int gfs_ctx_setup_nd(gfs_ctx *c, const gfs_layout_params *p, const gfs_launch_config *cfg,
                     const double *etas, const double *zetas) {
    if (!p) return fail(GFS_E_ARG, "params is null");
    if (p->dimensions < 1 || p->dimensions > GFS_MAX_DIMS) return fail(GFS_E_UNSUPPORTED, "dimensions must be 1..8");
    return setup_common(c, &p->sgd, (int)p->dimensions, cfg, etas, zetas);
}

uint64_t gfs_ctx_positions_len(const gfs_ctx *c) { return c ? c->x_len : 0; }

int gfs_ctx_upload_positions(gfs_ctx *c, const double *host, uint64_t n) {
    if (!c || !host) return fail(GFS_E_ARG, "null argument");
    if (!c->d_x) return fail(GFS_E_STATE, "context not set up");
    if (n != c->x_len) return fail(GFS_E_ARG, "positions length mismatch");
    HIPCHK(hipSetDevice(c->device));
    // device order: 1D x[slot]; nD the planes coords[end][dim][slot] — reordered on the device
    gfs::Buffer d_stage;
    if (int rc = d_stage.reserve(n * 8)) return rc;
    hipError_t e = hipMemcpy(d_stage.p, host, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gfs::reorder_positions_device(d_stage.as<double>(), c->d_x, c->d_perm, c->n_nodes, (uint32_t)c->dims, 1, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("upload_positions: ") + hipGetErrorString(e));
    return GFS_OK;
}
int gfs_ctx_init_positions(gfs_ctx *c) {                                  // K4, sgd.rs:286-294
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (!c->d_x || c->dims != 0) return fail(GFS_E_STATE, "needs a 1D context that has been set up");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    hipError_t e = gfs::init_positions_device(c->d_node_len, c->d_perm, c->d_x, c->n_nodes);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("init_positions: ") + hipGetErrorString(e));
    return GFS_OK;
}
int gfs_ctx_download_positions(gfs_ctx *c, double *host, uint64_t n) {
    if (!c || !host) return fail(GFS_E_ARG, "null argument");
    if (!c->d_x) return fail(GFS_E_STATE, "context not set up");
    if (n != c->x_len) return fail(GFS_E_ARG, "positions length mismatch");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    gfs::Buffer d_stage;
    if (int rc = d_stage.reserve(n * 8)) return rc;
    hipError_t e = gfs::reorder_positions_device(c->d_x, d_stage.as<double>(), c->d_perm, c->n_nodes, (uint32_t)c->dims, 0, 0);
    if (e == hipSuccess) e = hipMemcpy(host, d_stage.p, n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("download_positions: ") + hipGetErrorString(e));
    return GFS_OK;
}
int gfs_ctx_node_layout(const gfs_ctx *c, uint32_t *perm_out, uint64_t n) {
    if (!c || !perm_out) return fail(GFS_E_ARG, "null argument");
    if (n != c->n_nodes) return fail(GFS_E_ARG, "layout length mismatch");
    std::copy(c->perm.begin(), c->perm.end(), perm_out);
    return GFS_OK;
}
void *gfs_ctx_positions_device(gfs_ctx *c) { return c ? (void *)c->d_x : nullptr; }
int gfs_ctx_bind_positions(gfs_ctx *c, void *device_ptr) {
    if (!c || !device_ptr) return fail(GFS_E_ARG, "null argument");
    if (!c->configured || !c->x_len) return fail(GFS_E_STATE, "context not set up");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->d_x.borrow(device_ptr));                                     // (frees the context's own vector)
    return GFS_OK;
}
int gfs_ctx_reset_streams(gfs_ctx *c) {
    if (c && c->configured && !c->valid_paths) return GFS_NOTHING_TO_DO;
    if (!c || !c->d_rng) return fail(GFS_E_STATE, "context not set up");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    // Counters, team state and trace counts back to zero — a memset each: the traces, which stay, lie between them, and in a set's
    // arena other items' arrays — and the setup's seeding launch for this context alone, from the tables the setup left in the arena.
    const uint64_t T = c->shape.n_streams;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, kCounterBytes, 0));
    if (c->d_lead) HIPCHK(hipMemsetAsync(c->d_lead, 0, 8 * T * sizeof(uint32_t), 0));
    if (c->d_trace_cnt) HIPCHK(hipMemsetAsync(c->d_trace_cnt, 0, T * sizeof(uint32_t), 0));
    HIPCHK(gfs::seed_streams_device(c->d_seed_item, c->d_seed_blocks, (uint32_t)((T + gfs::SEED_BLOCK - 1) / gfs::SEED_BLOCK), 0));
    HIPCHK(hipDeviceSynchronize());
    c->events_used = 0; c->kernel_ms_harvested = 0.0; c->iterations = 0; c->total_ms = 0.0;
    return GFS_OK;
}

}  // extern "C"

void gfs::fill_kargs(const gfs_ctx *c, gfs::KArgs &a) {
    a.step_rec = c->d_step_rec; a.path_rec = c->d_path_rec; a.path_len = c->d_path_len;
    a.zetas = c->d_zetas; a.x = c->d_x; a.rng = c->d_rng; a.counters = c->d_counters;
    a.trace = c->d_trace; a.trace_cnt = c->d_trace_cnt; a.lead = c->d_lead;
    a.n_steps = c->n_steps;
    const bool wide = gfs::wide_index(c->n_steps, c->cfg.flags);
    a.steps_thresh = wide ? (0ull - c->n_steps) % c->n_steps
                          : (uint64_t)((uint32_t)(0u - (uint32_t)c->n_steps) % (uint32_t)c->n_steps);
    a.n_paths = (uint32_t)c->n_paths;
    a.zlen_full = (uint32_t)c->shape.zlen_full; a.zlen_staged = (uint32_t)c->shape.zlen_staged;
    a.n_streams = (uint32_t)c->shape.n_streams;
    a.quota_base = (uint32_t)(c->shape.quota_total / c->shape.n_streams);
    a.quota_rem = (uint32_t)(c->shape.quota_total % c->shape.n_streams);
    a.attempt_factor = (uint32_t)c->shape.attempt_factor;
    a.trace_per_stream = (uint32_t)c->cfg.trace_per_stream;
    a.space = (uint32_t)std::min<uint64_t>(c->params.space, 0xFFFFFFFFull);
    a.space_max = (uint32_t)std::min<uint64_t>(c->params.space_max, 0xFFFFFFFFull);
    a.space_q = (uint32_t)std::min<uint64_t>(c->params.space_quantization_step, 0xFFFFFFFFull);
    a.dbg = (c->cfg.flags >> 8) & 0x7Fu;             // bit 0x40 = GFS_F_DBG_WIDE_INDEX >> 8
    if (c->cfg.flags & GFS_F_DBG_NO_FUSED_TRIP) a.dbg |= 0x100u;     // (GFS_F_DBG_NO_TWIN_TRIP 0x400 arrives as dbg bit 0x04)
    a.bundle = c->shape.bundle;
    a.chain = c->shape.chain;
    a.partners = c->shape.partners;
    a.dbg2 = 0;
    if (const char *e = std::getenv("GFS_DBG2")) a.dbg2 = (uint32_t)std::atol(e);
    a.chunk = c->dims ? gfs::ND_TEAM_CHUNK : gfs::TEAM_CHUNK;
    a.ref_chunk = gfs::REF_CHUNK_PER_LANE;
    if (const char *e = std::getenv("GFS_DBG_REF_CHUNK")) { const long v = std::atol(e); if (v >= 1 && v <= 4096) a.ref_chunk = (uint32_t)v; }   // probe knob (scripts/ref_fused_probe.py)
    a.n_nodes = (uint32_t)c->n_nodes;
    a.kshift = c->kshift_override >= 0 ? c->kshift_override : gfs::crowd_kshift(c->n_steps, c->shape.n_streams);
    // (trip_rec shares the trace's word, sgd_device.h KArgs: a compact shape has no trace — compact_records — and is a team shape
    // at B = 64, which no batch takes: batch_eligible asks for reference streams)
    if (c->shape.compact) a.trip_rec = c->d_trip_rec;
}

extern "C" {

static int next_event_pair(gfs_ctx *c, gfs::EventPair *&ev) {
    if (c->events_used == c->events.size()) {
        if (c->events.size() >= 4096) {
            // long-lived context: recycle the pool instead of growing it (one sync per 4096 launches)
            HIPCHK(hipEventSynchronize(c->events.back().e1));
            for (auto &p : c->events) {
                float t = 0.f;
                if (p.elapsed(&t)) c->kernel_ms_harvested += t;
            }
            c->events_used = 0;
        } else {
            c->events.emplace_back();
            if (int rc = c->events.back().ready()) { c->events.pop_back(); return rc; }
        }
    }
    ev = &c->events[c->events_used++];
    return GFS_OK;
}

int gfs_ctx_run_iteration(gfs_ctx *c, uint64_t k, void *hip_stream) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (!c->configured) return fail(GFS_E_STATE, "context not set up");
    if (!c->valid_paths || c->n_nodes == 0) return GFS_NOTHING_TO_DO;
    if (k > c->params.iter_max) return fail(GFS_E_ARG, "iteration beyond iter_max");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    gfs::KArgs a{};
    fill_kargs(c, a);
    a.it = gfs::iter_consts(c, k);
    const bool window = gfs::in_window(c->shape, k);                                 // GFS_F_PHASED: the window's iterations are K1's
    if (window) a.bundle = 1;
    gfs::EventPair *ev = nullptr;
    int rc = next_event_pair(c, ev);
    if (rc) return rc;
    HIPCHK(ev->start(st));
    hipError_t e = launch(c, window ? c->plan.window_iteration : c->shape.compact ? c->plan.iteration_compact : c->plan.iteration, a, nullptr, 0, nullptr, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    HIPCHK(ev->stop(st));
    c->iterations++;
    c->launches++;
    return GFS_OK;
}

// A range of iterations ks[0..n) (each in 0..=iter_max): ONE fused launch for the team kernels (sgd1d_team_fused_kernel; layouts of 2
// and more dimensions at B = 64: sgdnd_team_fused_kernel) and for reference streams (sgd1d_fused_kernel, sgdnd_fused_kernel); otherwise one
// launch per iteration.  Which of the two, with which kernel, is the context's shape and plan (launch_policy.h, plan_launches); only
// the length of the range and the probe knobs are looked at here.
int gfs_ctx_run_range(gfs_ctx *c, const uint64_t *ks, uint64_t n, void *hip_stream) {
    if (!c || (!ks && n)) return fail(GFS_E_ARG, "null argument");
    if (!c->configured) return fail(GFS_E_STATE, "context not set up");
    if (!c->valid_paths || c->n_nodes == 0) return GFS_NOTHING_TO_DO;
    for (uint64_t i = 0; i < n; ++i) if (ks[i] > c->params.iter_max) return fail(GFS_E_ARG, "iteration beyond iter_max");
    const LaunchPlan &pl = c->plan;
    uint32_t one_chunk = c->shape.one_chunk;
    bool fuse_one = c->shape.fuse_one;
    if (const char *e = std::getenv("GFS_DBG_ONE_CHUNK")) {               // probe knob (scripts/one_iteration_launch_probe.py): also for the sort
        const long v = std::atol(e);
        if (v >= 64 && v <= 4096 && !(v & (v - 1))) { one_chunk = (uint32_t)v; fuse_one = c->shape.fuse_one_probe; }
    }
    if (!pl.fused || n == 0 || (n == 1 && !fuse_one) || n > 0xFFFFFFFFull) {
        for (uint64_t i = 0; i < n; ++i) { int rc = gfs_ctx_run_iteration(c, ks[i], hip_stream); if (rc) return rc; }
        return GFS_OK;
    }
    // a fused launch covers at most kMaxFusedIterations (its pool counters are 1 KB per iteration); longer ranges are
    // consecutive launches on the stream
    constexpr uint64_t kMaxFusedIterations = 4096;
    if (n > kMaxFusedIterations) {
        for (uint64_t off = 0; off < n; off += kMaxFusedIterations) {
            const uint64_t m = std::min(kMaxFusedIterations, n - off);
            int rc = m > 1 ? gfs_ctx_run_range(c, ks + off, m, hip_stream) : gfs_ctx_run_iteration(c, ks[off], hip_stream);
            if (rc) return rc;
        }
        return GFS_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    bool consecutive = c->d_its_all != nullptr;
    for (uint64_t i = 1; i < n && consecutive; ++i) consecutive = ks[i] == ks[0] + i;
    const gfs::IterConsts *d_slice = nullptr;
    if (consecutive) {
        d_slice = c->d_its_all + ks[0];               // resident table: nothing to upload, nothing to wait for
    } else {
        std::vector<gfs::IterConsts> its(n);
        for (uint64_t i = 0; i < n; ++i) its[i] = gfs::iter_consts(c, ks[i]);
        if (int rc = c->d_its.reserve(n * sizeof(gfs::IterConsts))) return rc;
        d_slice = c->d_its.as<gfs::IterConsts>();
        HIPCHK(hipMemcpyAsync(c->d_its.p, its.data(), n * sizeof(gfs::IterConsts), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));             // `its` is a stack-lifetime staging buffer
    }
    gfs::KArgs a{};
    fill_kargs(c, a);
    if (n == 1 && c->shape.bundle > 1) a.chunk = one_chunk;
    if (const char *e = std::getenv("GFS_DBG_CHUNK")) {                    // probe knob: the chunk of every fused team launch
        const long v = std::atol(e);
        if (c->shape.bundle > 1 && v >= 64 && v <= 16384 && !(v & (v - 1))) a.chunk = (uint32_t)v;
    }
    a.it = gfs::iter_consts(c, ks[0]);
    // work pools (sgd_kernel_common.h pool_walk): the waves draw an iteration's updates from shared counters, zeroed per launch
    uint32_t *pool = nullptr;
    if (c->shape.pooled) {
        if (int rc = c->d_pool.reserve(gfs::pool_bytes(n))) return rc;
        pool = c->d_pool.as<uint32_t>();
        HIPCHK(hipMemsetAsync(pool, 0, gfs::pool_bytes(n), st));
    }
    gfs::EventPair *ev = nullptr;
    int rc = next_event_pair(c, ev);
    if (rc) return rc;
    HIPCHK(ev->start(st));                // (the event pair brackets the kernel alone)
    hipError_t e = launch(c, c->shape.compact ? pl.fused_compact : pl.fused, a, d_slice, (uint32_t)n, pool, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("fused kernel launch: ") + hipGetErrorString(e));
    HIPCHK(ev->stop(st));
    c->iterations += n;
    c->launches++;
    return GFS_OK;
}

int gfs_ctx_synchronize(gfs_ctx *c, void *hip_stream) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    return GFS_OK;
}

int gfs_ctx_run(gfs_ctx *c, void *hip_stream) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (!c->configured) return fail(GFS_E_STATE, "context not set up");
    if (!c->valid_paths || c->n_nodes == 0) return GFS_NOTHING_TO_DO;
    auto t0 = std::chrono::steady_clock::now();
    {
        std::vector<uint64_t> ks(c->params.iter_max + 1);                  // iter_max+1 batches (sgd.rs:383)
        std::iota(ks.begin(), ks.end(), (uint64_t)0);
        int rc = gfs_ctx_run_range(c, ks.data(), ks.size(), hip_stream);
        if (rc) return rc;
    }
    int rc = gfs_ctx_synchronize(c, hip_stream);
    if (rc) return rc;
    c->total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GFS_OK;
}

int gfs_ctx_stats(gfs_ctx *c, gfs_stats *out) {
    if (!c || !out) return fail(GFS_E_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    if (!c->d_counters) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> cnt(kCounterBytes / 8);
    HIPCHK(hipMemcpy(cnt.data(), c->d_counters, kCounterBytes, hipMemcpyDeviceToHost));
    for (size_t s = 0; s < cnt.size(); s += 8) { out->term_updates += cnt[s]; out->attempts += cnt[s + 1]; }
    out->iterations = c->iterations; out->n_streams = c->shape.n_streams; out->bundle = c->shape.bundle; out->run_trips = c->shape.chain;
    double ms = c->kernel_ms_harvested;
    for (size_t k = 0; k < c->events_used; ++k) {
        float t = 0.f;
        if (c->events[k].elapsed(&t)) ms += t;
    }
    out->kernel_ms = ms; out->total_ms = c->total_ms; out->launches = c->launches;
    return GFS_OK;
}

int gfs_ctx_trace(gfs_ctx *c, gfs_term *out, uint64_t n_terms, uint64_t *counts, uint64_t n_streams) {
    if (!c || !out) return fail(GFS_E_ARG, "null argument");
    if (!c->d_trace) return fail(GFS_E_STATE, "trace_per_stream was 0");
    if (n_terms != c->shape.n_streams * c->cfg.trace_per_stream) return fail(GFS_E_ARG, "trace length mismatch");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->d_trace, n_terms * sizeof(gfs_term), hipMemcpyDeviceToHost));
    {   // the kernels record internal node indices: translate to the ABI's dense indices
        std::vector<uint32_t> inv(c->n_nodes);
        for (uint64_t k = 0; k < c->n_nodes; ++k) inv[c->perm[k]] = (uint32_t)k;
        for (uint64_t t = 0; t < n_terms; ++t) {
            if (c->dims == 0) { if (out[t].d_ij != 0.0) { out[t].i = inv[out[t].i]; out[t].j = inv[out[t].j]; } }
            else if (out[t].d_ij != 0.0) { out[t].i = inv[out[t].i >> 1] * 2 + (out[t].i & 1); out[t].j = inv[out[t].j >> 1] * 2 + (out[t].j & 1); }
        }
    }
    if (counts) {
        if (n_streams != c->shape.n_streams) return fail(GFS_E_ARG, "counts length mismatch");
        std::vector<uint32_t> tmp(c->shape.n_streams);
        HIPCHK(hipMemcpy(tmp.data(), c->d_trace_cnt, tmp.size() * 4, hipMemcpyDeviceToHost));
        for (uint64_t t = 0; t < c->shape.n_streams; ++t) counts[t] = tmp[t];
    }
    return GFS_OK;
}

// ---- test hooks ----
int gfs_ctx_debug_step_records(const gfs_ctx *c, uint32_t *out, uint64_t n_words) {
    if (!c || !out) return fail(GFS_E_ARG, "null argument");
    if (n_words != 4 * (c->n_steps + 1)) return fail(GFS_E_ARG, "step records length mismatch");
    if (!c->d_step_rec) return fail(GFS_E_STATE, "no step records");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->d_step_rec, (c->n_steps + 1) * sizeof(uint4), hipMemcpyDeviceToHost));
    return GFS_OK;
}
int gfs_ctx_debug_sgd_state(gfs_ctx *c, uint32_t which, void *out, uint64_t bytes) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    const uint32_t kind = which & ~GFS_STATE_SIZE_OF;
    if (kind >= GFS_STATE_KINDS) return fail(GFS_E_ARG, "no such state array");
    if (!c->configured) return fail(GFS_E_STATE, "context not set up");
    const void *arrays[GFS_STATE_KINDS] = {c->d_x.p, c->d_counters.p, c->d_lead.p, c->d_trace.p, c->d_trace_cnt.p, c->d_rng.p, c->d_zetas.p, c->d_its_all.p};
    const uint64_t size = arrays[kind] ? gfs::state_bytes(kind, c->d_rng.p != nullptr, c->x_len, c->shape, c->params, c->cfg) : 0;
    if (which & GFS_STATE_SIZE_OF) {
        if (!out || bytes != sizeof(uint64_t)) return fail(GFS_E_ARG, "the size of a state array is one uint64_t");
        *static_cast<uint64_t *>(out) = size;
        return GFS_OK;
    }
    if (bytes != size) return fail(GFS_E_ARG, "state array length mismatch: it has " + std::to_string(size) + " bytes");
    if (!size) return GFS_OK;
    if (!out) return fail(GFS_E_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, arrays[kind], size, hipMemcpyDeviceToHost));
    return GFS_OK;
}
int gfs_ctx_debug_kshift(gfs_ctx *c, int32_t set, int32_t *kshift_out) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (set >= -1) {
        c->kshift_override = set;
        if (c->configured && c->shape.n_streams)                           // the record width follows the onset (launch_policy.h)
            gfs::shape_records(c->record_facts, set >= 0 ? set : gfs::crowd_kshift(c->n_steps, c->shape.n_streams), &c->shape);
    }                                                                      // (set < -1: a query only)
    if (kshift_out) {
        if (!c->configured || !c->shape.n_streams) return fail(GFS_E_STATE, "context not set up");
        gfs::KArgs a{};
        fill_kargs(c, a);
        *kshift_out = a.kshift;
    }
    return GFS_OK;
}

uint32_t gfs_ctx_record_bytes(const gfs_ctx *c) {
    if (!c || !c->configured || !c->shape.n_streams) return 0;
    return c->shape.compact ? (uint32_t)sizeof(uint2) : (uint32_t)sizeof(uint4);
}

int gfs_ctx_phase_window(gfs_ctx *c, int64_t set_begin, int64_t set_end, uint64_t *begin_out, uint64_t *end_out) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (!c->configured || !(c->cfg.flags & GFS_F_PHASED)) return fail(GFS_E_STATE, "context not set up with GFS_F_PHASED");
    if (set_begin >= 0 || set_end >= 0) {
        if (set_begin < 0 || set_end < 0 || set_begin > set_end || (uint64_t)set_end > c->params.iter_max + 1)
            return fail(GFS_E_ARG, "phase window: need 0 <= begin <= end <= iter_max + 1");
        if (!c->shape.phased) return fail(GFS_E_STATE, "GFS_F_PHASED is a no-op on this context (the auto policy did not pick bundles of 64)");
        c->shape.win_begin = (uint64_t)set_begin; c->shape.win_end = (uint64_t)set_end;
        if (c->d_its_all) {                                                // the resident schedule carries the window's marks
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipDeviceSynchronize());
            int rc = upload_schedule(c);
            if (rc) return rc;
        }
    }
    if (begin_out) *begin_out = c->shape.win_begin;
    if (end_out) *end_out = c->shape.win_end;
    return GFS_OK;
}

// K6 on the device: rank order of the context's current positions (1D) — sgd.rs:665-671.
int gfs_ctx_sort_order(gfs_ctx *c, uint64_t *order, uint64_t n) {
    if (!c || (!order && n)) return fail(GFS_E_ARG, "null argument");
    if (!c->d_x || c->dims != 0) return fail(GFS_E_STATE, "needs a 1D context that has been set up");
    if (n != c->n_nodes) return fail(GFS_E_ARG, "order length mismatch");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    gfs::Buffer d_tmp;
    if (int rc = d_tmp.reserve(gfs::sort_order_scratch_bytes(n))) return rc;
    uint32_t *d_order = nullptr;
    hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, d_tmp.p, &d_order);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("sort_order_device: ") + hipGetErrorString(e));
    std::vector<uint32_t> tmp(n);
    e = hipMemcpy(tmp.data(), d_order, n * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("hipMemcpy order: ") + hipGetErrorString(e));
    for (uint64_t k = 0; k < n; ++k) order[k] = tmp[k];
    return GFS_OK;
}

// ---- K7: quality read-outs of the resident positions (quality_kernels.hip) --------------------------------------------
// (their scratch is gfs_ctx::d_quality, in 8-byte words)
}  // extern "C"

int gfs::check_step_distances(const uint64_t *zs, uint64_t n_z, const gfs_pair_error *out) {
    if ((!zs || !out) && n_z) return fail(GFS_E_ARG, "null argument");
    if (n_z > 65535) return fail(GFS_E_ARG, "at most 65535 step distances per call");
    for (uint64_t k = 0; k < n_z; ++k) if (zs[k] == 0) return fail(GFS_E_ARG, "a step distance of 0");
    return GFS_OK;
}
int gfs::check_diagnosis(uint64_t z, double ratio) {
    if (z == 0) return fail(GFS_E_ARG, "a step distance of 0");
    if (!(ratio >= 0.0)) return fail(GFS_E_ARG, "ratio must be a number >= 0");
    return GFS_OK;
}
gfs_pair_error gfs::unpack_pair_error(uint64_t z, const uint64_t *w) {
    gfs_pair_error o{};
    o.step_distance = z; o.pairs = w[0];
    std::memcpy(&o.sum_rel_sq, &w[1], 8); std::memcpy(&o.max_rel_sq, &w[2], 8);
    std::memcpy(&o.sum_abs, &w[3], 8); std::memcpy(&o.sum_sq, &w[4], 8);
    return o;
}
gfs_sort_quality gfs::unpack_sort_quality(const uint64_t *w) {
    gfs_sort_quality o{w[0], w[1], w[2], 0.0};
    std::memcpy(&o.sq_err_sum, &w[3], 8);
    return o;
}
int gfs::check_sorted_length(uint64_t total_bp, int64_t batch_item) {
    if (total_bp < (1ull << 53)) return GFS_OK;
    return fail(GFS_E_UNSUPPORTED, (batch_item < 0 ? "" : "batch item " + std::to_string(batch_item) + ": ") + "a graph of 2^53 bp or more");
}

extern "C" {

static uint64_t *scratch_words(const gfs_ctx *c, uint64_t part) { return gfs::Region::at<uint64_t>(c->d_quality.p, part); }   // a part of an entry's map
// the duration of an entry's device work on stderr under GFS_TIMING: only then does the entry's event pair come into being
static void start_if_timing(gfs::EventPair &timer, hipStream_t st) { if (std::getenv("GFS_TIMING")) (void)timer.start(st); }
// after the stream was synchronised; `count` is a step distance, or (before = "", after = " step distances") how many there were
static void report_timing(const gfs::EventPair &timer, const char *what, uint64_t count, uint64_t n_steps, const char *before = "z = ", const char *after = "") {
    float ms = 0.f;
    if (timer.elapsed(&ms))
        std::fprintf(stderr, "[%s] %s%llu%s, %llu steps: kernels %.4f ms\n", what, before, (unsigned long long)count, after,
                     (unsigned long long)n_steps, ms);
}

int gfs_ctx_pair_errors(gfs_ctx *c, const uint64_t *zs, uint64_t n_z, gfs_pair_error *out, void *hip_stream) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    int rc = gfs::check_step_distances(zs, n_z, out);
    if (rc) return rc;
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_z == 0) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t blocks = gfs::quality_blocks(c->n_steps);
    gfs::Region map;                                                       // scratch: [zs | out words | partials]
    const uint64_t zs_at = map.add(8 * n_z), out_at = map.add(8 * 5 * n_z), partials_at = map.add(8 * 5 * n_z * blocks);
    if ((rc = c->d_quality.reserve(map.bytes()))) return rc;
    uint64_t *d_zs = scratch_words(c, zs_at), *d_out = scratch_words(c, out_at), *d_partials = scratch_words(c, partials_at);
    HIPCHK(hipMemcpyAsync(d_zs, zs, n_z * 8, hipMemcpyHostToDevice, st));
    gfs::EventPair timer;
    start_if_timing(timer, st);
    hipError_t e = gfs::pair_errors_device(c->d_step_rec, c->n_steps, c->d_x, c->n_nodes, (uint32_t)c->dims, d_zs, (uint32_t)n_z,
                                           d_partials, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("pair_errors_device: ") + hipGetErrorString(e));
    (void)timer.stop(st);
    std::vector<uint64_t> w(5 * n_z);
    HIPCHK(hipMemcpyAsync(w.data(), d_out, w.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    report_timing(timer, "gfs_ctx_pair_errors", n_z, c->n_steps, "", " step distances");
    for (uint64_t k = 0; k < n_z; ++k) out[k] = gfs::unpack_pair_error(zs[k], &w[5 * k]);
    return GFS_OK;
}

int gfs_ctx_stress_of_pairs(gfs_ctx *c, const uint64_t *step_a, const uint64_t *step_b, uint64_t n, double *rel_sq_out,
                            uint64_t *counted, double *stress) {
    if (!c || !counted || !stress || ((!step_a || !step_b) && n)) return fail(GFS_E_ARG, "null argument");
    *counted = 0; *stress = 0.0;
    for (uint64_t i = 0; i < n; ++i)
        if (step_a[i] >= c->n_steps || step_b[i] >= c->n_steps) return fail(GFS_E_ARG, "a step index beyond n_steps");
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n == 0) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    gfs::Region map;                                                       // scratch: [step_a | step_b | rel_sq]
    const uint64_t a_at = map.add(8 * n), b_at = map.add(8 * n), rel_at = map.add(8 * n);
    if (int rc = c->d_quality.reserve(map.bytes())) return rc;
    uint64_t *d_a = scratch_words(c, a_at), *d_b = scratch_words(c, b_at);
    double *d_rel = map.at<double>(c->d_quality.p, rel_at);
    HIPCHK(hipMemcpy(d_a, step_a, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_b, step_b, n * 8, hipMemcpyHostToDevice));
    hipError_t e = gfs::pair_list_device(c->d_step_rec, c->n_steps, c->d_x, c->n_nodes, (uint32_t)c->dims, d_a, d_b, n, d_rel, nullptr);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("pair_list_device: ") + hipGetErrorString(e));
    std::vector<double> own;
    double *rel = rel_sq_out;
    if (!rel) { own.resize(n); rel = own.data(); }
    HIPCHK(hipMemcpy(rel, d_rel, n * 8, hipMemcpyDeviceToHost));
    double sum = 0.0; uint64_t cnt = 0;                                    // in sample order: sgd.rs:1274-1275
    for (uint64_t i = 0; i < n; ++i) if (rel[i] >= 0.0) { sum += rel[i]; ++cnt; }
    *counted = cnt;
    *stress = cnt ? std::sqrt(sum / (double)cnt) : 0.0;                    // :1278-1282
    return GFS_OK;
}

int gfs_ctx_sort_quality(gfs_ctx *c, gfs_sort_quality *out) {
    if (!c || !out) return fail(GFS_E_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    if (!c->d_x || c->dims != 0) return fail(GFS_E_STATE, "needs a 1D context that has been set up");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    const uint64_t n = c->n_nodes, blocks = gfs::quality_blocks(c->n_steps);
    gfs::Buffer d_sort;
    int rc = d_sort.reserve(gfs::sort_order_scratch_bytes(n));
    if (rc) return rc;
    uint32_t *d_order = nullptr;
    hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, d_sort.p, &d_order);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("sort_order_device: ") + hipGetErrorString(e));
    gfs::Region map;                                                       // scratch: [prefix | sorted positions | partials | out]
    const uint64_t prefix_at = map.add(8 * (n + 1)), spos_at = map.add(8 * n), partials_at = map.add(8 * 5 * blocks), out_at = map.add(8 * 5);
    if ((rc = c->d_quality.reserve(map.bytes()))) return rc;
    uint64_t *d_prefix = scratch_words(c, prefix_at), *d_spos = scratch_words(c, spos_at), *d_partials = scratch_words(c, partials_at);
    uint64_t *d_out = scratch_words(c, out_at);
    uint64_t total_len = 0;
    e = gfs::sort_quality_device(c->d_step_rec, c->n_steps, d_order, c->d_node_len, c->d_perm, n, d_prefix, d_spos, d_partials, d_out,
                                 &total_len, nullptr);
    d_sort.reset();
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("sort_quality_device: ") + hipGetErrorString(e));
    if ((rc = gfs::check_sorted_length(total_len))) return rc;
    uint64_t w[5];
    HIPCHK(hipMemcpy(w, d_out, sizeof w, hipMemcpyDeviceToHost));
    *out = gfs::unpack_sort_quality(w);
    return GFS_OK;
}

// ---- K7d / K7e / K7f: per path, per stretched pair, per node ------------------------------------------------------------
int gfs_ctx_path_errors(gfs_ctx *c, uint64_t z, double ratio, gfs_path_error *out, uint64_t n_paths, void *hip_stream) {
    if (!c || (!out && n_paths)) return fail(GFS_E_ARG, "null argument");
    int rc = gfs::check_diagnosis(z, ratio);
    if (rc) return rc;
    if (n_paths != c->n_paths) return fail(GFS_E_ARG, "n_paths does not match the context");
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_paths == 0) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t tiles = gfs::quality_tiles(c->n_steps);
    gfs::Region map;                                                       // scratch: [out | head partials | tail partials]
    const uint64_t out_at = map.add(n_paths * sizeof(gfs_path_error)), head_at = map.add(8 * 5 * tiles), tail_at = map.add(8 * 5 * tiles);
    if ((rc = c->d_quality.reserve(map.bytes()))) return rc;
    uint64_t *d_out = scratch_words(c, out_at), *d_head = scratch_words(c, head_at), *d_tail = scratch_words(c, tail_at);
    gfs::EventPair timer;
    start_if_timing(timer, st);
    hipError_t e = gfs::path_errors_device(c->d_step_rec, c->n_steps, c->d_path_rec, n_paths, c->d_x, c->n_nodes, (uint32_t)c->dims, z, ratio,
                                           d_head, d_tail, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("path_errors_device: ") + hipGetErrorString(e));
    (void)timer.stop(st);
    HIPCHK(hipMemcpyAsync(out, d_out, n_paths * sizeof(gfs_path_error), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    report_timing(timer, "gfs_ctx_path_errors", z, c->n_steps);
    return GFS_OK;
}

int gfs_ctx_stretched_pairs(gfs_ctx *c, uint64_t z, double ratio, gfs_stretched_pair *out, uint64_t cap, uint64_t *total,
                            void *hip_stream) {
    if (!c || !total || (!out && cap)) return fail(GFS_E_ARG, "null argument");
    *total = 0;
    int rc = gfs::check_diagnosis(z, ratio);
    if (rc) return rc;
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t tiles = gfs::quality_tiles(c->n_steps), room = std::min(cap, c->n_steps);
    gfs::Region map;                                                       // scratch: [tile counts | offsets | list]
    const uint64_t counts_at = map.add(8 * (tiles + 1)), offsets_at = map.add(8 * (tiles + 1)), list_at = map.add(room * sizeof(gfs_stretched_pair));
    if ((rc = c->d_quality.reserve(map.bytes()))) return rc;
    uint64_t *d_counts = scratch_words(c, counts_at), *d_offsets = scratch_words(c, offsets_at), *d_list = scratch_words(c, list_at);
    gfs::EventPair timer;
    start_if_timing(timer, st);
    hipError_t e = gfs::stretched_pairs_device(c->d_step_rec, c->n_steps, c->d_x, c->n_nodes, (uint32_t)c->dims, z, ratio, d_counts, d_offsets,
                                               room ? d_list : nullptr, room, total, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("stretched_pairs_device: ") + hipGetErrorString(e));
    (void)timer.stop(st);
    const uint64_t n = std::min(room, *total);
    if (n) HIPCHK(hipMemcpyAsync(out, d_list, n * sizeof(gfs_stretched_pair), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    report_timing(timer, "gfs_ctx_stretched_pairs", z, c->n_steps);
    return GFS_OK;
}

int gfs_ctx_node_errors(gfs_ctx *c, uint64_t z, double ratio, gfs_node_error *out, uint64_t n_nodes, void *hip_stream) {
    if (!c || (!out && n_nodes)) return fail(GFS_E_ARG, "null argument");
    int rc = gfs::check_diagnosis(z, ratio);
    if (rc) return rc;
    if (n_nodes != c->n_nodes) return fail(GFS_E_ARG, "n_nodes does not match the context");
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_nodes == 0) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    gfs::Region map;                                                       // scratch: [per slot: pairs | stretched | max] [out]
    const uint64_t slots_at = map.add(n_nodes * sizeof(gfs_node_error)), out_at = map.add(n_nodes * sizeof(gfs_node_error));
    if ((rc = c->d_quality.reserve(map.bytes()))) return rc;
    uint64_t *d_slots = scratch_words(c, slots_at), *d_out = scratch_words(c, out_at);
    gfs::EventPair timer;
    start_if_timing(timer, st);
    hipError_t e = gfs::node_errors_device(c->d_step_rec, c->n_steps, c->d_x, c->d_perm, n_nodes, (uint32_t)c->dims, z, ratio, d_slots, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("node_errors_device: ") + hipGetErrorString(e));
    (void)timer.stop(st);
    HIPCHK(hipMemcpyAsync(out, d_out, n_nodes * sizeof(gfs_node_error), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    report_timing(timer, "gfs_ctx_node_errors", z, c->n_steps);
    return GFS_OK;
}

// ---- multi-GPU replica merge helpers (device pointers, asynchronous on hip_stream) -----------------
int gfs_merge_prepare(const double *x, const double *x_prev, float *buf2n, uint64_t n, void *hip_stream) {
    if (!x || !x_prev || !buf2n) return fail(GFS_E_ARG, "null argument");
    if (n == 0) return GFS_OK;
    hipError_t e = gfs::launch_merge_prepare(x, x_prev, buf2n, n, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("merge_prepare: ") + hipGetErrorString(e));
    return GFS_OK;
}
int gfs_merge_apply(double *x, double *x_prev, const float *buf2n, uint64_t n, double divide_all_by, void *hip_stream) {
    if (!x || !x_prev || !buf2n) return fail(GFS_E_ARG, "null argument");
    if (n == 0) return GFS_OK;
    hipError_t e = gfs::launch_merge_apply(x, x_prev, buf2n, n, divide_all_by, (hipStream_t)hip_stream);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("merge_apply: ") + hipGetErrorString(e));
    return GFS_OK;
}

// ---- one-shot entry points -------------------------------------------------------------------
static int one_shot(const gfs_graph_view *g, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg,
                    const double *etas, const double *zetas, int init_x, double *x, gfs_stats *stats,
                    uint64_t *order = nullptr) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (!g || !p) return fail(GFS_E_ARG, "null argument");
    if (g->n_nodes == 0) return GFS_NOTHING_TO_DO;                         // sgd.rs:242-244,780-782
    if (!x) return fail(GFS_E_ARG, "positions buffer is null");
    gfs::Laps laps{"gfasort_hip", true};                                        // phase times of the one-shot call on stderr
    gfs_ctx *c = nullptr;
    int rc = gfs_ctx_create(g, 0, &c);
    if (rc) return rc;
    laps.lap("ctx_create");
    if (dims == 0) rc = gfs_ctx_setup_1d(c, p, cfg, etas, zetas);
    else { gfs_layout_params lp; lp.dimensions = (uint64_t)dims; lp.sgd = *p; rc = gfs_ctx_setup_nd(c, &lp, cfg, etas, zetas); }
    if (rc) { gfs_ctx_destroy(c); return rc; }
    laps.lap("setup");
    if (dims == 0 && init_x) rc = gfs_ctx_init_positions(c);             // K4 on the device
    else rc = gfs_ctx_upload_positions(c, x, gfs_ctx_positions_len(c));
    laps.lap("upload");
    if (!rc) rc = gfs_ctx_run(c, nullptr);
    laps.lap("run");
    if (!rc) rc = gfs_ctx_download_positions(c, x, gfs_ctx_positions_len(c));
    laps.lap("download");
    if (!rc && order) { rc = gfs_ctx_sort_order(c, order, g->n_nodes); laps.lap("sort"); }
    if (!rc && stats) {
        rc = gfs_ctx_stats(c, stats);
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - laps.t).count();
    }
    gfs_ctx_destroy(c);
    laps.lap("destroy");
    return rc;
}

// A finished result measured without a run: a context that holds positions and nothing else (no schedule, no streams).
static int positions_only_ctx(const gfs_graph_view *g, uint64_t dims, const double *positions, gfs_ctx **out) {
    gfs_ctx *c = nullptr;
    int rc = gfs_ctx_create(g, 0, &c);
    if (rc) return rc;
    c->dims = (int)dims;
    c->x_len = dims ? c->n_nodes * 2 * dims : c->n_nodes;
    rc = c->d_x.reserve(c->x_len * 8, "hipMalloc positions");
    if (!rc) rc = gfs_ctx_upload_positions(c, positions, c->x_len);
    if (rc) { gfs_ctx_destroy(c); return rc; }
    *out = c;
    return GFS_OK;
}

int gfs_pair_errors(const gfs_graph_view *g, uint64_t dims, const double *positions, const uint64_t *zs, uint64_t n_z,
                    gfs_pair_error *out) {
    if (!g) return fail(GFS_E_ARG, "null argument");
    int rc = gfs::check_step_distances(zs, n_z, out);
    if (rc) return rc;
    if (dims > GFS_MAX_DIMS) return fail(GFS_E_ARG, "dims must be 0 (1D positions) or 1..8");
    for (uint64_t k = 0; k < n_z; ++k) { out[k] = gfs_pair_error{}; out[k].step_distance = zs[k]; }
    if (g->n_nodes == 0) return GFS_NOTHING_TO_DO;
    if (!positions) return fail(GFS_E_ARG, "positions buffer is null");
    gfs_ctx *c = nullptr;
    rc = positions_only_ctx(g, dims, positions, &c);
    if (rc) return rc;
    rc = gfs_ctx_pair_errors(c, zs, n_z, out, nullptr);
    gfs_ctx_destroy(c);
    return rc;
}

int gfs_sort_quality_of(const gfs_graph_view *g, const double *positions, gfs_sort_quality *out) {
    if (!g || !out) return fail(GFS_E_ARG, "null argument");
    if (g->n_nodes && !positions) return fail(GFS_E_ARG, "positions buffer is null");
    *out = gfs_sort_quality{};
    if (g->n_nodes == 0) return GFS_NOTHING_TO_DO;
    gfs_ctx *c = nullptr;
    int rc = positions_only_ctx(g, 0, positions, &c);
    if (rc) return rc;
    rc = gfs_ctx_sort_quality(c, out);
    gfs_ctx_destroy(c);
    return rc;
}

int gfs_diagnose(const gfs_graph_view *g, uint64_t dims, const double *positions, uint64_t z, double ratio,
                 gfs_path_error *paths_out, gfs_stretched_pair *pairs_out, uint64_t cap, uint64_t *total) {
    if (!g || !total || (!paths_out && g->n_paths) || (!pairs_out && cap)) return fail(GFS_E_ARG, "null argument");
    *total = 0;
    int rc = gfs::check_diagnosis(z, ratio);
    if (rc) return rc;
    if (dims > GFS_MAX_DIMS) return fail(GFS_E_ARG, "dims must be 0 (1D positions) or 1..8");
    for (uint64_t p = 0; p < g->n_paths; ++p) paths_out[p] = gfs_path_error{};
    if (g->n_nodes == 0) return GFS_NOTHING_TO_DO;
    if (!positions) return fail(GFS_E_ARG, "positions buffer is null");
    gfs_ctx *c = nullptr;
    rc = positions_only_ctx(g, dims, positions, &c);
    if (rc) return rc;
    rc = gfs_ctx_path_errors(c, z, ratio, paths_out, g->n_paths, nullptr);
    if (!rc) rc = gfs_ctx_stretched_pairs(c, z, ratio, pairs_out, cap, total, nullptr);
    gfs_ctx_destroy(c);
    return rc;
}

int gfs_path_linear_sgd(const gfs_graph_view *g, const gfs_sgd_params *p, const gfs_launch_config *cfg,
                        const double *etas, const double *zetas, int init_x, double *x_inout, gfs_stats *stats) {
    return one_shot(g, p, 0, cfg, etas, zetas, init_x, x_inout, stats);
}

int gfs_path_sgd_sort(const gfs_graph_view *g, const gfs_sgd_params *p, const gfs_launch_config *cfg,
                      const double *etas, const double *zetas, int init_x, double *x_inout, uint64_t *order_out,
                      gfs_stats *stats) {
    if (!order_out) return fail(GFS_E_ARG, "order buffer is null");
    return one_shot(g, p, 0, cfg, etas, zetas, init_x, x_inout, stats, order_out);
}

int gfs_path_linear_sgd_layout(const gfs_graph_view *g, const gfs_layout_params *p, const gfs_launch_config *cfg,
                               const double *etas, const double *zetas, double *coords_inout, gfs_stats *stats) {
    if (!p) return fail(GFS_E_ARG, "params is null");
    if (p->dimensions < 1 || p->dimensions > GFS_MAX_DIMS) return fail(GFS_E_UNSUPPORTED, "dimensions must be 1..8");
    return one_shot(g, &p->sgd, (int)p->dimensions, cfg, etas, zetas, 0, coords_inout, stats);
}

}  // extern "C"
