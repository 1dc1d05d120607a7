// capi.hip — the device plumbing of the C ABI of libgfasort_hip.so (include/gfasort_hip.h): the resident
// context (device mirror of PathIndex + positions + RNG streams), its launches and read-outs, batches, and the one-shot entry
// points that stand where path_linear_sgd / path_linear_sgd_layout stand in the reference.  What a context launches is decided in
// launch_policy.h; the host tables are host_tables.hip's.
#include "../../include/gfasort_hip.h"
#include "sgd_kernel_common.h"
#include "sgd_batch.h"
#include "batch_plan.h"
#include "batch_readout_plan.h"
#include "segment_sort.h"
#include "launch_policy.h"
#include "sgd_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

static int fail(int code, const std::string &msg) { return gfs_set_error(code, msg); }   // (the error slot: host_tables.hip)
#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(GFS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
    } while (0)

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
    const bool timing = std::getenv("GFS_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(GFS_E_HIP, "no HIP device available (libgfasort_hip has no CPU fallback)");
    if (device < 0 || device >= n) return fail(GFS_E_ARG, "bad device index");
    auto lap = [&](const char *what) {
        if (!timing) return;
        auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[gfs_warmup] %-12s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(nullptr));
    lap("context");
    // code objects load on first use, one per translation unit: touch each now, and the allocator too
    HIPCHK(gfs::warm_module_1d());
    HIPCHK(gfs::warm_module_1d_phased());
    lap("module 1d");
    HIPCHK(gfs::warm_module_index());
    HIPCHK(gfs::warm_module_quality());
    lap("module index");
    HIPCHK(gfs::warm_module_nd());
    HIPCHK(gfs::warm_module_nd_team());
    HIPCHK(gfs::warm_module_nd_team_wide());
    lap("modules nd");
    // ... and the copy paths in both directions (the first hipMemcpy of a process sets up its staging
    // buffers and DMA queues: ~0.13 s when it was left to the first upload)
    void *p = nullptr;
    std::vector<unsigned char> h(1 << 20, 0);
    HIPCHK(hipMalloc(&p, 64u << 20));
    lap("malloc");
    HIPCHK(hipMemcpy(p, h.data(), h.size(), hipMemcpyHostToDevice));
    lap("h2d");
    HIPCHK(hipMemset(p, 0, 64u << 20));
    HIPCHK(hipDeviceSynchronize());
    lap("memset");
    HIPCHK(hipMemcpy(h.data(), p, h.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipDeviceSynchronize());
    lap("d2h");
    HIPCHK(hipFree(p));
    lap("free");
    return GFS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// resident context
// ---------------------------------------------------------------------------------------------
static constexpr size_t kCounterBytes = gfs::COUNTER_SLOTS * 8 * sizeof(unsigned long long);   // lines of 64 B

// The kernels of a configured context, resolved once by setup_common for the shape the policy decided (gfs_ctx::shape,
// launch_policy.h): everything of gfs_ctx_run_iteration / gfs_ctx_run_range that does not depend on the call.
struct LaunchPlan {
    const void *iteration = nullptr;         // K1 / K1b, K2 / K2b: one iteration per launch
    const void *window_iteration = nullptr;  // GFS_F_PHASED: K1, for the iterations of the window
    const void *fused = nullptr;             // K1c / K1d / K1e / K2c / K2d: a range of iterations per launch; null: one launch per iteration
};

struct gfs_ctx {
    int device = 0;
    int cu_count = 0;
    uint64_t n_nodes = 0, n_steps = 0, n_paths = 0;
    uint32_t max_path_steps = 0;
    bool valid_paths = false;
    std::vector<uint32_t> path_counts;
    std::vector<uint32_t> perm;        // dense node index (ABI order) -> internal index (device layout of positions)
    // device mirror of PathIndex
    uint4 *d_step_rec = nullptr;
    uint4 *d_path_rec = nullptr;
    uint64_t *d_path_len = nullptr;
    uint32_t *d_perm = nullptr;         // node layout on the device (dense index -> slot)
    uint32_t *d_node_len = nullptr;     // node lengths by dense index (K4: initial positions)
    // SGD state
    int dims = 0;                      // 0 = 1D
    bool configured = false;
    gfs_sgd_params params{};
    gfs_launch_config cfg{};
    std::vector<double> etas;
    double *d_zetas = nullptr;
    double *d_x = nullptr; bool x_owned = false; uint64_t x_len = 0;
    uint64_t *d_rng = nullptr;
    uint32_t *d_lead = nullptr;      // team kernels: the waves' partly expanded passes, [8][n_streams]
    unsigned long long *d_counters = nullptr;
    gfs_term *d_trace = nullptr; uint32_t *d_trace_cnt = nullptr;
    gfs::IterConsts *d_its = nullptr; uint64_t its_cap = 0;   // schedule slice of a fused launch (arbitrary lists)
    gfs::IterConsts *d_its_all = nullptr;                     // constants of iterations 0..=iter_max, resident
    uint32_t *d_pool = nullptr; uint64_t pool_cap = 0;        // fused launch: per-iteration work pool counters (sgd_kernels_1d.hip)
    gfs::LaunchShape shape;            // streams, bundle, run length, phase window, LDS tables, what a range launches (launch_policy.h)
    LaunchPlan plan;
    int32_t kshift_override = -1;      // test hook gfs_ctx_debug_kshift: >= 0 replaces the crowding onset of fill_kargs
    uint64_t *d_quality = nullptr; uint64_t quality_cap = 0;   // K7 read-outs: scratch in 8-byte words, kept between calls
    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    double kernel_ms_harvested = 0.0;  // durations of event pairs already recycled
    uint64_t iterations = 0;
    uint64_t launches = 0;
    double total_ms = 0.0;
};

static void free_sgd_state(gfs_ctx *c) {
    if (c->d_zetas) (void)hipFree(c->d_zetas);
    if (c->d_x && c->x_owned) (void)hipFree(c->d_x);
    if (c->d_rng) (void)hipFree(c->d_rng);
    if (c->d_lead) (void)hipFree(c->d_lead);
    c->d_lead = nullptr;
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->d_trace) (void)hipFree(c->d_trace);
    if (c->d_trace_cnt) (void)hipFree(c->d_trace_cnt);
    if (c->d_its) (void)hipFree(c->d_its);
    if (c->d_its_all) (void)hipFree(c->d_its_all);
    c->d_its = nullptr; c->its_cap = 0; c->d_its_all = nullptr;
    if (c->d_pool) (void)hipFree(c->d_pool);
    c->d_pool = nullptr; c->pool_cap = 0;
    c->d_zetas = nullptr; c->d_x = nullptr; c->d_rng = nullptr; c->d_counters = nullptr;
    c->d_trace = nullptr; c->d_trace_cnt = nullptr; c->x_owned = false; c->configured = false;
}

static int seed_streams(gfs_ctx *c) {
    // stream t <- Xoshiro256Plus::seed_from_u64(seed + stream_base + t)   (sgd.rs:431-432)
    const uint64_t T = c->shape.n_streams;
    std::vector<uint64_t> st(4 * T);
    for (uint64_t t = 0; t < T; ++t) {
        uint64_t sm = c->params.seed + c->cfg.stream_base + t;
        for (int k = 0; k < 4; ++k) st[(uint64_t)k * T + t] = gfs::splitmix64(sm);
    }
    HIPCHK(hipMemcpy(c->d_rng, st.data(), st.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(c->d_counters, 0, kCounterBytes));
    if (c->d_trace_cnt) HIPCHK(hipMemset(c->d_trace_cnt, 0, T * sizeof(uint32_t)));
    c->events_used = 0; c->kernel_ms_harvested = 0.0; c->iterations = 0; c->total_ms = 0.0;
    return GFS_OK;
}

// The zeta table of sgd.rs:311-331 on the device.  Only indices reachable from
// jump <= min(space, max_path_steps-1) are ever read (sgd.rs:462-469: shape.zlen_staged of them); when the table is computed here
// the running sum — which is order-dependent and must be accumulated exactly as the reference does —
// stops at the largest i that feeds a reachable entry (space is the longest path in bp: 1.3e6 for C3,
// of which 1.6e5 matter).
static int upload_zeta_table(gfs_ctx *c, const gfs_sgd_params *p, const double *zetas) {
    const uint64_t zlen_full = c->shape.zlen_full;
    std::vector<double> ztab;
    if (!zetas) {
        const uint64_t m = c->shape.zlen_staged - 1;                // last staged index
        const uint64_t need_i = m <= p->space_max ? m : p->space_max + (m - p->space_max - 1) * p->space_quantization_step;
        gfs_sgd_params q = *p;
        q.space = std::min<uint64_t>(p->space, std::max<uint64_t>(need_i, 1));
        std::vector<double> part(gfs_zeta_table_len(&q));
        gfs_zeta_table(&q, part.data());
        ztab.assign(zlen_full, 0.0);
        std::copy(part.begin(), part.begin() + std::min<size_t>(part.size(), ztab.size()), ztab.begin());
        zetas = ztab.data();
    }
    HIPCHK(hipMalloc(&c->d_zetas, zlen_full * 8));
    HIPCHK(hipMemcpy(c->d_zetas, zetas, zlen_full * 8, hipMemcpyHostToDevice));
    return GFS_OK;
}

static gfs::IterConsts iter_consts(const gfs_ctx *c, uint64_t k) { return gfs::iter_consts(c->params, c->etas, c->shape, k); }

// The resident table of the whole schedule's constants (d_its_all); again whenever the phase window moves, whose marks it carries.
static int upload_schedule(gfs_ctx *c) {
    std::vector<gfs::IterConsts> all(c->params.iter_max + 1);
    for (uint64_t k = 0; k <= c->params.iter_max; ++k) all[k] = iter_consts(c, k);
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
static int resident_blocks_per_cu(const gfs_ctx *c, const void *fn, int *per_cu) {
    hipFuncAttributes attr;
    HIPCHK(hipFuncGetAttributes(&attr, fn));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, (int)c->shape.block, c->shape.lds_bytes));
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

// Resolves c->plan for c->shape as shape_before_residency left it, asks the runtime for the fused team kernel's residency and
// lets shape_after_residency finish the shape (which may lower n_streams).
static int plan_launches(gfs_ctx *c) {
    gfs::LaunchShape &s = c->shape;
    LaunchPlan &pl = c->plan;
    pl = LaunchPlan{};
    const gfs::KernelShape shape{s.dims, s.bundle, s.lds_tables, s.atomic_loads, s.trace};
    const bool team = s.team, ref = s.bundle == 1;
    const bool free_running = (s.flags & GFS_F_DBG_FREE_RUNNING) != 0;
    pl.iteration = iteration_kernel(shape);
    if (s.phased) pl.window_iteration = iteration_kernel({0, 1, s.lds_tables, s.atomic_loads, s.trace});
    const void *pooled_kernel = s.phased ? gfs::phased_fused_kernel(s.lds_tables) : (team || ref) ? fused_kernel(shape, true) : nullptr;
    const void *free_kernel = team && !s.phased && free_running ? fused_kernel(shape, false) : nullptr;   // (K1e, K1d, K2d: pools only)
    if (!pl.iteration || (s.phased && !pl.window_iteration) || ((team || ref) && !pooled_kernel) ||
        (team && !s.phased && free_running && !free_kernel))
        return fail(GFS_E_UNSUPPORTED, "no kernel is built for dims=" + std::to_string(s.dims) + " bundle=" + std::to_string(s.bundle) +
                                           " lds_tables=" + std::to_string(s.lds_tables) + " atomic_loads=" + std::to_string(s.atomic_loads) +
                                           " trace=" + std::to_string(s.trace) + " phased=" + std::to_string(s.phased));
    int per_cu = 0;
    if (team) {                                                            // (the measurement behind it: shape_after_residency)
        int rc = resident_blocks_per_cu(c, pooled_kernel, &per_cu);
        if (rc) return rc;
    }
    gfs::shape_after_residency(per_cu, gfs::DeviceFacts{c->cu_count}, &s);
    if (s.fused) pl.fused = s.pooled ? pooled_kernel : free_kernel;
    return GFS_OK;
}

static int setup_common(gfs_ctx *c, const gfs_sgd_params *p, int dims, const gfs_launch_config *cfg,
                        const double *etas, const double *zetas) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    std::string err;
    int rc = gfs::check_setup_args(p, dims, cfg, &err);                    // (refused before the context is touched)
    if (rc) return fail(rc, err);
    HIPCHK(hipSetDevice(c->device));
    free_sgd_state(c);
    c->shape = gfs::LaunchShape{};
    c->plan = LaunchPlan{};
    c->params = *p;
    c->cfg = cfg ? *cfg : gfs_launch_config{};
    c->dims = dims;
    c->x_len = 0;
    if (c->n_nodes == 0) { c->configured = true; return GFS_NOTHING_TO_DO; }

    // positions.  A context with nothing to do (no path of more than one step: sgd.rs:250-261 returns before any
    // update) still owns a full-length position replica: a multi-GPU rank whose shard holds no such path must be able to
    // upload, bind, merge and download like its peers — its contribution to every merge is a zero delta of the same size.
    c->x_len = dims ? c->n_nodes * 2 * (uint64_t)dims : c->n_nodes;
    HIPCHK(hipMalloc(&c->d_x, c->x_len * 8));
    HIPCHK(hipMemset(c->d_x, 0, c->x_len * 8));
    c->x_owned = true;
    if (!c->valid_paths) { c->configured = true; return GFS_NOTHING_TO_DO; }

    // launch shape (launch_policy.h): decided before anything of the run's state is allocated
    const gfs::GraphFacts graph{c->n_nodes, c->n_steps, c->n_paths, c->max_path_steps, c->valid_paths, c->path_counts.data()};
    rc = gfs::shape_before_residency(graph, gfs::DeviceFacts{c->cu_count}, p, dims, cfg, &c->shape, &err);
    if (rc) return fail(rc, err);
    rc = plan_launches(c);                                               // (may lower n_streams)
    if (rc) return rc;
    const uint64_t n_streams = c->shape.n_streams;

    // eta schedule and zeta table (host, bit-exact) unless supplied
    c->etas.resize(p->iter_max + 1);
    if (etas) std::copy(etas, etas + p->iter_max + 1, c->etas.begin());
    else gfs_sgd_schedule(p, c->etas.data());
    rc = upload_zeta_table(c, p, zetas);
    if (rc) return rc;

    HIPCHK(hipMalloc(&c->d_rng, 4 * n_streams * 8));
    if (c->shape.bundle > 1) {                                           // team kernels, sort and layout
        HIPCHK(hipMalloc(&c->d_lead, 8 * n_streams * sizeof(uint32_t)));
        HIPCHK(hipMemset(c->d_lead, 0, 8 * n_streams * sizeof(uint32_t)));      // trips left = 0: no pass yet
    }
    HIPCHK(hipMalloc(&c->d_counters, kCounterBytes));
    if (c->cfg.trace_per_stream) {
        HIPCHK(hipMalloc(&c->d_trace, n_streams * c->cfg.trace_per_stream * sizeof(gfs_term)));
        HIPCHK(hipMemset(c->d_trace, 0, n_streams * c->cfg.trace_per_stream * sizeof(gfs_term)));
        HIPCHK(hipMalloc(&c->d_trace_cnt, n_streams * sizeof(uint32_t)));
    }
    rc = seed_streams(c);
    if (rc) return rc;
    if ((c->shape.team || c->shape.bundle == 1) && c->params.iter_max < (1u << 20)) {
        // the whole schedule's per-iteration constants, for fused launches over consecutive iterations
        HIPCHK(hipMalloc(&c->d_its_all, (c->params.iter_max + 1) * sizeof(gfs::IterConsts)));
        rc = upload_schedule(c);
        if (rc) return rc;
    }
    c->configured = true;
    return GFS_OK;
}

extern "C" {

int gfs_ctx_create(const gfs_graph_view *g, int device, gfs_ctx **out) {
    return gfs_ctx_create_with_layout(g, device, nullptr, out);
}

int gfs_ctx_create_with_layout(const gfs_graph_view *g, int device, const uint32_t *node_perm, gfs_ctx **out) {
    if (!g || !out) return fail(GFS_E_ARG, "null argument");
    *out = nullptr;
    if (g->n_steps > (1ull << 40)) return fail(GFS_E_UNSUPPORTED, "more than 2^40 path steps");
    if (g->n_nodes > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "more than 2^31-1 nodes");
    if (g->n_paths > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "more than 2^31-1 paths");
    if (g->n_steps && (!g->step_node || !g->step_is_rev)) return fail(GFS_E_ARG, "null step arrays");
    if (!g->path_first_step) return fail(GFS_E_ARG, "null path_first_step");
    if (g->n_nodes && !g->node_len) return fail(GFS_E_ARG, "null node_len");
    if (g->path_first_step[0] != 0 || g->path_first_step[g->n_paths] != g->n_steps)
        return fail(GFS_E_ARG, "path_first_step must start at 0 and end at n_steps");
    for (uint64_t p = 0; p < g->n_paths; ++p)
        if (g->path_first_step[p + 1] < g->path_first_step[p]) return fail(GFS_E_ARG, "path_first_step not monotone");
    // (step_node's range is checked on the device, in the pass that derives the node layout)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GFS_E_HIP, "no HIP device available (libgfasort_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFS_E_ARG, "bad device index");
    const bool timing = std::getenv("GFS_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[gfs_ctx_create] %-12s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    lap("validate");
    gfs_ctx *c = new (std::nothrow) gfs_ctx();
    if (!c) return fail(GFS_E_NOMEM, "out of memory");
    c->device = device;
    c->n_nodes = g->n_nodes; c->n_steps = g->n_steps; c->n_paths = g->n_paths;
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete c; return fail(GFS_E_HIP, "hipGetDeviceProperties failed");
    }
    c->cu_count = prop.multiProcessorCount;

    // Internal node layout.  The position vector is stored in FIRST-VISIT PATH ORDER (nodes in the
    // order the paths first step on them, unvisited nodes last; derived on the device, index_kernels.hip)
    // unless the caller supplies a layout: consecutive steps of a path then touch neighbouring position words whatever the
    // order of the input's S lines was, which is what lets a run's loads and atomics coalesce
    // (C3 with randomly ordered nodes: 63 G updates/s in path order, 11 G/s in input order).
    c->perm.assign(g->n_nodes, 0xFFFFFFFFu);
    if (node_perm) {
        std::vector<uint8_t> seen(g->n_nodes, 0);
        for (uint64_t k = 0; k < g->n_nodes; ++k) {
            if (node_perm[k] >= g->n_nodes || seen[node_perm[k]]) { delete c; return fail(GFS_E_ARG, "node_perm is not a permutation"); }
            seen[node_perm[k]] = 1; c->perm[k] = node_perm[k];
        }
    }
    // Path records (host, P entries) and the facts the launch logic needs
    std::vector<uint4> prec(std::max<uint64_t>(g->n_paths, 1));
    for (uint64_t p = 0; p < g->n_paths; ++p) {
        uint64_t b = g->path_first_step[p], e = g->path_first_step[p + 1];
        uint32_t cnt = (uint32_t)(e - b);
        if (e - b > 0xFFFFFFFFull) { delete c; return fail(GFS_E_UNSUPPORTED, "a path with more than 2^32-1 steps"); }
        prec[p].x = (uint32_t)b; prec[p].y = cnt;
        prec[p].z = cnt ? (uint32_t)(0u - cnt) % cnt : 0u; prec[p].w = (uint32_t)(b >> 32);
        c->path_counts.push_back(cnt);
        if (cnt > 1) c->valid_paths = true;                               // sgd.rs:250-256
        c->max_path_steps = std::max(c->max_path_steps, cnt);
    }
    {   // a step record keeps 55 bits of a step's bp position (its top bits carry the crowding exponents): refuse longer paths
        // instead of truncating them.  Cheap bound first (steps x longest node), the exact sum only where that fails.
        uint32_t max_len = 0;
        for (uint64_t k = 0; k < g->n_nodes; ++k) max_len = std::max(max_len, g->node_len[k]);
        for (uint64_t p = 0; p < g->n_paths; ++p) {
            const uint64_t b = g->path_first_step[p], e2 = g->path_first_step[p + 1];
            if ((unsigned __int128)(e2 - b) * max_len < ((unsigned __int128)1 << 55)) continue;
            unsigned __int128 bp = 0;
            for (uint64_t s2 = b; s2 < e2; ++s2) { const uint32_t n = g->step_node[s2]; if (n < g->n_nodes) bp += g->node_len[n]; }
            if (bp >= ((unsigned __int128)1 << 55)) { delete c; return fail(GFS_E_UNSUPPORTED, "a path of 2^55 bp or more"); }
        }
    }
    // K3 on the device: PathIndex::from_graph (sgd.rs:34-71) — the per-path exclusive prefix sum of
    // node lengths over the steps — written straight into the 16-byte step records
    // (index_kernels.hip).  Uploads 5 B per step instead of 16.
    auto bail = [&](const char *what, hipError_t e) {
        std::string m = std::string(what) + ": " + hipGetErrorString(e);
        gfs_ctx_destroy(c);
        return fail(GFS_E_HIP, m);
    };
    const uint64_t S = g->n_steps, N = g->n_nodes, P = g->n_paths;
    uint32_t *d_step_node = nullptr; uint8_t *d_rev = nullptr; uint64_t *d_first = nullptr, *d_tmp = nullptr;
    auto free_tmp = [&]() {
        if (d_step_node) (void)hipFree(d_step_node);
        if (d_rev) (void)hipFree(d_rev); if (d_first) (void)hipFree(d_first); if (d_tmp) (void)hipFree(d_tmp);
    };
    hipError_t e;
#define GFS_TRY(what, expr) if ((e = (expr)) != hipSuccess) { free_tmp(); return bail(what, e); }
    // (one record of padding, zeroed: the layout team kernels read the record AFTER a step for its node's length and use it
    // only where that step is not its path's last — so the graph's very last step needs no clamp, sgd_kernels_nd_team.hip)
    GFS_TRY("hipMalloc step_rec", hipMalloc(&c->d_step_rec, (S + 1) * sizeof(uint4)));
    GFS_TRY("hipMemset step_rec", hipMemset(c->d_step_rec + S, 0, sizeof(uint4)));
    GFS_TRY("hipMalloc path_rec", hipMalloc(&c->d_path_rec, prec.size() * sizeof(uint4)));
    GFS_TRY("hipMalloc path_len", hipMalloc(&c->d_path_len, std::max<uint64_t>(P, 1) * 8));
    GFS_TRY("hipMalloc perm", hipMalloc(&c->d_perm, std::max<uint64_t>(N, 1) * 4));
    GFS_TRY("hipMalloc node_len", hipMalloc(&c->d_node_len, std::max<uint64_t>(N, 1) * 4));
    if (N) { GFS_TRY("hipMemcpy node_len", hipMemcpy(c->d_node_len, g->node_len, N * 4, hipMemcpyHostToDevice)); }
    GFS_TRY("hipMemcpy path_rec", hipMemcpy(c->d_path_rec, prec.data(), prec.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if (S) {
        GFS_TRY("hipMalloc step_node", hipMalloc(&d_step_node, S * 4));
        GFS_TRY("hipMemcpy step_node", hipMemcpy(d_step_node, g->step_node, S * 4, hipMemcpyHostToDevice));
    }
    if (S) {
        GFS_TRY("hipMalloc path_first", hipMalloc(&d_first, (P + 1) * 8));
        GFS_TRY("hipMemcpy path_first", hipMemcpy(d_first, g->path_first_step, (P + 1) * 8, hipMemcpyHostToDevice));
    }
    lap("step upload");
    {
        // range check of step_node, and (unless the caller brought a layout) the first-visit order
        int bad = 0;
        uint32_t *d_scratch_perm = nullptr;
        uint32_t *target = c->d_perm;
        if (node_perm && N) { GFS_TRY("hipMalloc scratch", hipMalloc(&d_scratch_perm, N * 4)); target = d_scratch_perm; }
        e = gfs::first_visit_layout_device(d_step_node, S, N, d_first, (uint32_t)P, target, &bad);
        if (d_scratch_perm) (void)hipFree(d_scratch_perm);
        if (e != hipSuccess) { free_tmp(); return bail("first_visit_layout", e); }
        if (bad) { free_tmp(); gfs_ctx_destroy(c); return fail(GFS_E_ARG, "step_node out of range"); }
        if (N && node_perm) { GFS_TRY("hipMemcpy perm", hipMemcpy(c->d_perm, c->perm.data(), N * 4, hipMemcpyHostToDevice)); }
        if (N && !node_perm) { GFS_TRY("hipMemcpy perm", hipMemcpy(c->perm.data(), c->d_perm, N * 4, hipMemcpyDeviceToHost)); }
    }
    lap("node layout");
    if (S) {
        GFS_TRY("hipMalloc step_is_rev", hipMalloc(&d_rev, S));

        GFS_TRY("hipMalloc scan", hipMalloc(&d_tmp, (S + 1) * 8));
        lap("alloc tmp");
        GFS_TRY("hipMemcpy step_is_rev", hipMemcpy(d_rev, g->step_is_rev, S, hipMemcpyHostToDevice));

        lap("upload");
        GFS_TRY("build_path_index", gfs::build_path_index_device(d_step_node, d_rev, c->d_node_len, c->d_perm, d_first, (uint32_t)P, S, N,
                                                                  d_tmp, c->d_step_rec, c->d_path_len));
    }
#undef GFS_TRY
    lap("K3");
    free_tmp();
    lap("free tmp");
    *out = c;
    return GFS_OK;
}

void gfs_ctx_destroy(gfs_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    free_sgd_state(c);
    for (auto &ev : c->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (c->d_step_rec) (void)hipFree(c->d_step_rec);
    if (c->d_path_rec) (void)hipFree(c->d_path_rec);
    if (c->d_path_len) (void)hipFree(c->d_path_len);
    if (c->d_perm) (void)hipFree(c->d_perm);
    if (c->d_node_len) (void)hipFree(c->d_node_len);
    if (c->d_quality) (void)hipFree(c->d_quality);
    delete c;
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
    double *d_stage = nullptr;
    HIPCHK(hipMalloc(&d_stage, n * 8));
    hipError_t e = hipMemcpy(d_stage, host, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gfs::reorder_positions_device(d_stage, c->d_x, c->d_perm, c->n_nodes, (uint32_t)c->dims, 1, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(d_stage);
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
    double *d_stage = nullptr;
    HIPCHK(hipMalloc(&d_stage, n * 8));
    hipError_t e = gfs::reorder_positions_device(c->d_x, d_stage, c->d_perm, c->n_nodes, (uint32_t)c->dims, 0, 0);
    if (e == hipSuccess) e = hipMemcpy(host, d_stage, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_stage);
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
    if (c->d_x && c->x_owned) HIPCHK(hipFree(c->d_x));
    c->d_x = (double *)device_ptr; c->x_owned = false;
    return GFS_OK;
}
int gfs_ctx_reset_streams(gfs_ctx *c) {
    if (c && c->configured && !c->valid_paths) return GFS_NOTHING_TO_DO;
    if (!c || !c->d_rng) return fail(GFS_E_STATE, "context not set up");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    if (c->d_lead) HIPCHK(hipMemset(c->d_lead, 0, 8 * c->shape.n_streams * sizeof(uint32_t)));
    return seed_streams(c);
}

static void fill_kargs(const gfs_ctx *c, gfs::KArgs &a) {
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
}

static int next_event_pair(gfs_ctx *c, std::pair<hipEvent_t, hipEvent_t> *&ev) {
    if (c->events_used == c->events.size()) {
        if (c->events.size() >= 4096) {
            // long-lived context: recycle the pool instead of growing it (one sync per 4096 launches)
            HIPCHK(hipEventSynchronize(c->events.back().second));
            for (auto &p : c->events) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, p.first, p.second) == hipSuccess) c->kernel_ms_harvested += t;
            }
            c->events_used = 0;
        } else {
            hipEvent_t e0, e1;
            HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
            c->events.emplace_back(e0, e1);
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
    a.it = iter_consts(c, k);
    const bool window = gfs::in_window(c->shape, k);                                 // GFS_F_PHASED: the window's iterations are K1's
    if (window) a.bundle = 1;
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    int rc = next_event_pair(c, ev);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev->first, st));
    hipError_t e = launch(c, window ? c->plan.window_iteration : c->plan.iteration, a, nullptr, 0, nullptr, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    HIPCHK(hipEventRecord(ev->second, st));
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
        for (uint64_t i = 0; i < n; ++i) its[i] = iter_consts(c, ks[i]);
        if (c->its_cap < n) {
            if (c->d_its) HIPCHK(hipFree(c->d_its));
            c->d_its = nullptr; c->its_cap = 0;
            HIPCHK(hipMalloc(&c->d_its, n * sizeof(gfs::IterConsts)));
            c->its_cap = n;
        }
        HIPCHK(hipMemcpyAsync(c->d_its, its.data(), n * sizeof(gfs::IterConsts), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));             // `its` is a stack-lifetime staging buffer
        d_slice = c->d_its;
    }
    gfs::KArgs a{};
    fill_kargs(c, a);
    if (n == 1 && c->shape.bundle > 1) a.chunk = one_chunk;
    if (const char *e = std::getenv("GFS_DBG_CHUNK")) {                    // probe knob: the chunk of every fused team launch
        const long v = std::atol(e);
        if (c->shape.bundle > 1 && v >= 64 && v <= 16384 && !(v & (v - 1))) a.chunk = (uint32_t)v;
    }
    a.it = iter_consts(c, ks[0]);
    // work pools (sgd_kernel_common.h pool_walk): the waves draw an iteration's updates from shared counters, zeroed per launch
    uint32_t *pool = nullptr;
    if (c->shape.pooled) {
        if (c->pool_cap < n) {
            if (c->d_pool) HIPCHK(hipFree(c->d_pool));
            c->d_pool = nullptr; c->pool_cap = 0;
            HIPCHK(hipMalloc(&c->d_pool, gfs::pool_bytes(n)));
            c->pool_cap = n;
        }
        HIPCHK(hipMemsetAsync(c->d_pool, 0, gfs::pool_bytes(n), st));
        pool = c->d_pool;
    }
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    int rc = next_event_pair(c, ev);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev->first, st));                // (the event pair brackets the kernel alone)
    hipError_t e = launch(c, pl.fused, a, d_slice, (uint32_t)n, pool, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("fused kernel launch: ") + hipGetErrorString(e));
    HIPCHK(hipEventRecord(ev->second, st));
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
        if (hipEventElapsedTime(&t, c->events[k].first, c->events[k].second) == hipSuccess) ms += t;
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
int gfs_ctx_debug_kshift(gfs_ctx *c, int32_t set, int32_t *kshift_out) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    if (set >= -1) c->kshift_override = set;                              // (set < -1: a query only)
    if (kshift_out) {
        if (!c->configured || !c->shape.n_streams) return fail(GFS_E_STATE, "context not set up");
        gfs::KArgs a{};
        fill_kargs(c, a);
        *kshift_out = a.kshift;
    }
    return GFS_OK;
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
    void *d_tmp = nullptr;
    HIPCHK(hipMalloc(&d_tmp, n * (2 * 8 + 2 * 4)));
    uint32_t *d_order = nullptr;
    hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, d_tmp, &d_order);
    if (e != hipSuccess) { (void)hipFree(d_tmp); return fail(GFS_E_HIP, std::string("sort_order_device: ") + hipGetErrorString(e)); }
    std::vector<uint32_t> tmp(n);
    e = hipMemcpy(tmp.data(), d_order, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_tmp);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("hipMemcpy order: ") + hipGetErrorString(e));
    for (uint64_t k = 0; k < n; ++k) order[k] = tmp[k];
    return GFS_OK;
}

// ---- K7: quality read-outs of the resident positions (quality_kernels.hip) --------------------------------------------
static int quality_scratch(gfs_ctx *c, uint64_t words) {
    if (c->quality_cap >= words) return GFS_OK;
    if (c->d_quality) HIPCHK(hipFree(c->d_quality));
    c->d_quality = nullptr; c->quality_cap = 0;
    HIPCHK(hipMalloc(&c->d_quality, words * 8));
    c->quality_cap = words;
    return GFS_OK;
}
static int check_step_distances(const uint64_t *zs, uint64_t n_z, const gfs_pair_error *out) {
    if ((!zs || !out) && n_z) return fail(GFS_E_ARG, "null argument");
    if (n_z > 65535) return fail(GFS_E_ARG, "at most 65535 step distances per call");
    for (uint64_t k = 0; k < n_z; ++k) if (zs[k] == 0) return fail(GFS_E_ARG, "a step distance of 0");
    return GFS_OK;
}
// the duration of an entry's device work on stderr under GFS_TIMING (one HIP event pair, destroyed however the entry returns)
struct QualityTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    explicit QualityTimer(hipStream_t s) : st(s) {
        if (!std::getenv("GFS_TIMING")) return;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, st) != hipSuccess) done();
    }
    void stop() { if (e0 && hipEventRecord(e1, st) != hipSuccess) done(); }
    bool elapsed(float *ms) const { return e0 && hipEventElapsedTime(ms, e0, e1) == hipSuccess; }   // after the stream was synchronised
    void report(const char *what, uint64_t z, uint64_t n_steps) const {
        float ms = 0.f;
        if (elapsed(&ms))
            std::fprintf(stderr, "[%s] z = %llu, %llu steps: kernels %.4f ms\n", what, (unsigned long long)z, (unsigned long long)n_steps, ms);
    }
    void done() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); e0 = e1 = nullptr; }
    ~QualityTimer() { done(); }
};

int gfs_ctx_pair_errors(gfs_ctx *c, const uint64_t *zs, uint64_t n_z, gfs_pair_error *out, void *hip_stream) {
    if (!c) return fail(GFS_E_ARG, "ctx is null");
    int rc = check_step_distances(zs, n_z, out);
    if (rc) return rc;
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_z == 0) return GFS_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t blocks = gfs::quality_blocks(c->n_steps);
    // scratch: [zs | out words | partials]
    rc = quality_scratch(c, n_z + 5 * n_z + 5 * n_z * blocks);
    if (rc) return rc;
    uint64_t *d_zs = c->d_quality, *d_out = d_zs + n_z, *d_partials = d_out + 5 * n_z;
    HIPCHK(hipMemcpyAsync(d_zs, zs, n_z * 8, hipMemcpyHostToDevice, st));
    QualityTimer timer(st);
    hipError_t e = gfs::pair_errors_device(c->d_step_rec, c->n_steps, c->d_x, c->n_nodes, (uint32_t)c->dims, d_zs, (uint32_t)n_z,
                                           d_partials, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("pair_errors_device: ") + hipGetErrorString(e));
    timer.stop();
    std::vector<uint64_t> w(5 * n_z);
    HIPCHK(hipMemcpyAsync(w.data(), d_out, w.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    if (timer.elapsed(&ms))
        std::fprintf(stderr, "[gfs_ctx_pair_errors] %llu step distances, %llu steps: kernels %.4f ms\n", (unsigned long long)n_z,
                     (unsigned long long)c->n_steps, ms);
    for (uint64_t k = 0; k < n_z; ++k) {
        out[k].step_distance = zs[k]; out[k].pairs = w[5 * k];
        std::memcpy(&out[k].sum_rel_sq, &w[5 * k + 1], 8); std::memcpy(&out[k].max_rel_sq, &w[5 * k + 2], 8);
        std::memcpy(&out[k].sum_abs, &w[5 * k + 3], 8); std::memcpy(&out[k].sum_sq, &w[5 * k + 4], 8);
    }
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
    int rc = quality_scratch(c, 3 * n);                                    // [step_a | step_b | rel_sq]
    if (rc) return rc;
    uint64_t *d_a = c->d_quality, *d_b = d_a + n;
    double *d_rel = reinterpret_cast<double *>(d_b + n);
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
    void *d_sort = nullptr;
    HIPCHK(hipMalloc(&d_sort, n * (2 * 8 + 2 * 4)));
    uint32_t *d_order = nullptr;
    hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, d_sort, &d_order);
    int rc = e == hipSuccess ? quality_scratch(c, (n + 1) + n + 5 * blocks + 5)      // [prefix | sorted positions | partials | out]
                             : fail(GFS_E_HIP, std::string("sort_order_device: ") + hipGetErrorString(e));
    if (rc) { (void)hipFree(d_sort); return rc; }
    uint64_t *d_prefix = c->d_quality, *d_spos = d_prefix + n + 1, *d_partials = d_spos + n, *d_out = d_partials + 5 * blocks;
    uint64_t total_len = 0;
    e = gfs::sort_quality_device(c->d_step_rec, c->n_steps, d_order, c->d_node_len, c->d_perm, n, d_prefix, d_spos, d_partials, d_out,
                                 &total_len, nullptr);
    (void)hipFree(d_sort);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("sort_quality_device: ") + hipGetErrorString(e));
    if (total_len >= (1ull << 53)) return fail(GFS_E_UNSUPPORTED, "a graph of 2^53 bp or more");
    uint64_t w[5];
    HIPCHK(hipMemcpy(w, d_out, sizeof w, hipMemcpyDeviceToHost));
    out->steps = w[0]; out->abs_err_sum = w[1]; out->genomic_sum = w[2];
    std::memcpy(&out->sq_err_sum, &w[3], 8);
    return GFS_OK;
}

// ---- K7d / K7e / K7f: per path, per stretched pair, per node ------------------------------------------------------------
static int check_diagnosis(uint64_t z, double ratio) {
    if (z == 0) return fail(GFS_E_ARG, "a step distance of 0");
    if (!(ratio >= 0.0)) return fail(GFS_E_ARG, "ratio must be a number >= 0");
    return GFS_OK;
}
int gfs_ctx_path_errors(gfs_ctx *c, uint64_t z, double ratio, gfs_path_error *out, uint64_t n_paths, void *hip_stream) {
    if (!c || (!out && n_paths)) return fail(GFS_E_ARG, "null argument");
    int rc = check_diagnosis(z, ratio);
    if (rc) return rc;
    if (n_paths != c->n_paths) return fail(GFS_E_ARG, "n_paths does not match the context");
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_paths == 0) return GFS_OK;
    static_assert(sizeof(gfs_path_error) == 8 * 8, "K7d writes gfs_path_error as 8 words");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t tiles = gfs::quality_tiles(c->n_steps);
    rc = quality_scratch(c, 8 * n_paths + 10 * tiles);                     // [out | head partials | tail partials]
    if (rc) return rc;
    uint64_t *d_out = c->d_quality, *d_head = d_out + 8 * n_paths, *d_tail = d_head + 5 * tiles;
    QualityTimer timer(st);
    hipError_t e = gfs::path_errors_device(c->d_step_rec, c->n_steps, c->d_path_rec, n_paths, c->d_x, c->n_nodes, (uint32_t)c->dims, z, ratio,
                                           d_head, d_tail, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("path_errors_device: ") + hipGetErrorString(e));
    timer.stop();
    HIPCHK(hipMemcpyAsync(out, d_out, n_paths * sizeof(gfs_path_error), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    timer.report("gfs_ctx_path_errors", z, c->n_steps);
    return GFS_OK;
}

int gfs_ctx_stretched_pairs(gfs_ctx *c, uint64_t z, double ratio, gfs_stretched_pair *out, uint64_t cap, uint64_t *total,
                            void *hip_stream) {
    if (!c || !total || (!out && cap)) return fail(GFS_E_ARG, "null argument");
    *total = 0;
    int rc = check_diagnosis(z, ratio);
    if (rc) return rc;
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    static_assert(sizeof(gfs_stretched_pair) == 5 * 8, "K7e writes gfs_stretched_pair as 5 words");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t tiles = gfs::quality_tiles(c->n_steps), room = std::min(cap, c->n_steps);
    rc = quality_scratch(c, 2 * (tiles + 1) + 5 * room);                   // [tile counts | offsets | list]
    if (rc) return rc;
    uint64_t *d_counts = c->d_quality, *d_offsets = d_counts + tiles + 1, *d_list = d_offsets + tiles + 1;
    QualityTimer timer(st);
    hipError_t e = gfs::stretched_pairs_device(c->d_step_rec, c->n_steps, c->d_x, c->n_nodes, (uint32_t)c->dims, z, ratio, d_counts, d_offsets,
                                               room ? d_list : nullptr, room, total, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("stretched_pairs_device: ") + hipGetErrorString(e));
    timer.stop();
    const uint64_t n = std::min(room, *total);
    if (n) HIPCHK(hipMemcpyAsync(out, d_list, n * sizeof(gfs_stretched_pair), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    timer.report("gfs_ctx_stretched_pairs", z, c->n_steps);
    return GFS_OK;
}

int gfs_ctx_node_errors(gfs_ctx *c, uint64_t z, double ratio, gfs_node_error *out, uint64_t n_nodes, void *hip_stream) {
    if (!c || (!out && n_nodes)) return fail(GFS_E_ARG, "null argument");
    int rc = check_diagnosis(z, ratio);
    if (rc) return rc;
    if (n_nodes != c->n_nodes) return fail(GFS_E_ARG, "n_nodes does not match the context");
    if (!c->d_x) return fail(GFS_E_STATE, "the context has no positions (not set up)");
    if (n_nodes == 0) return GFS_OK;
    static_assert(sizeof(gfs_node_error) == 3 * 8, "K7f writes gfs_node_error as 3 words");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    rc = quality_scratch(c, 6 * n_nodes);                                  // [per slot: pairs | stretched | max] [out]
    if (rc) return rc;
    uint64_t *d_slots = c->d_quality, *d_out = d_slots + 3 * n_nodes;
    QualityTimer timer(st);
    hipError_t e = gfs::node_errors_device(c->d_step_rec, c->n_steps, c->d_x, c->d_perm, n_nodes, (uint32_t)c->dims, z, ratio, d_slots, d_out, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("node_errors_device: ") + hipGetErrorString(e));
    timer.stop();
    HIPCHK(hipMemcpyAsync(out, d_out, n_nodes * sizeof(gfs_node_error), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    timer.report("gfs_ctx_node_errors", z, c->n_steps);
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
    auto t0 = std::chrono::steady_clock::now();
    const bool timing = std::getenv("GFS_TIMING") != nullptr;        // phase times of the one-shot call on stderr
    auto lap = [&](const char *what) {
        if (timing) std::fprintf(stderr, "[gfasort_hip] %-10s %8.2f ms\n", what,
                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    gfs_ctx *c = nullptr;
    int rc = gfs_ctx_create(g, 0, &c);
    if (rc) return rc;
    lap("ctx_create");
    if (dims == 0) rc = gfs_ctx_setup_1d(c, p, cfg, etas, zetas);
    else { gfs_layout_params lp; lp.dimensions = (uint64_t)dims; lp.sgd = *p; rc = gfs_ctx_setup_nd(c, &lp, cfg, etas, zetas); }
    if (rc) { gfs_ctx_destroy(c); return rc; }
    lap("setup");
    if (dims == 0 && init_x) rc = gfs_ctx_init_positions(c);             // K4 on the device
    else rc = gfs_ctx_upload_positions(c, x, gfs_ctx_positions_len(c));
    lap("upload");
    if (!rc) rc = gfs_ctx_run(c, nullptr);
    lap("run");
    if (!rc) rc = gfs_ctx_download_positions(c, x, gfs_ctx_positions_len(c));
    lap("download");
    if (!rc && order) { rc = gfs_ctx_sort_order(c, order, g->n_nodes); lap("sort"); }
    if (!rc && stats) {
        rc = gfs_ctx_stats(c, stats);
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    gfs_ctx_destroy(c);
    lap("destroy");
    return rc;
}

// A finished result measured without a run: a context that holds positions and nothing else (no schedule, no streams).
static int positions_only_ctx(const gfs_graph_view *g, uint64_t dims, const double *positions, gfs_ctx **out) {
    gfs_ctx *c = nullptr;
    int rc = gfs_ctx_create(g, 0, &c);
    if (rc) return rc;
    c->dims = (int)dims;
    c->x_len = dims ? c->n_nodes * 2 * dims : c->n_nodes;
    hipError_t e = hipMalloc(&c->d_x, c->x_len * 8);
    if (e != hipSuccess) { gfs_ctx_destroy(c); return fail(GFS_E_HIP, std::string("hipMalloc positions: ") + hipGetErrorString(e)); }
    c->x_owned = true;
    rc = gfs_ctx_upload_positions(c, positions, c->x_len);
    if (rc) { gfs_ctx_destroy(c); return rc; }
    *out = c;
    return GFS_OK;
}

int gfs_pair_errors(const gfs_graph_view *g, uint64_t dims, const double *positions, const uint64_t *zs, uint64_t n_z,
                    gfs_pair_error *out) {
    if (!g) return fail(GFS_E_ARG, "null argument");
    int rc = check_step_distances(zs, n_z, out);
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

int gfs_diagnose(const gfs_graph_view *g, uint64_t dims, const double *positions, uint64_t z, double ratio,
                 gfs_path_error *paths_out, gfs_stretched_pair *pairs_out, uint64_t cap, uint64_t *total) {
    if (!g || !total || (!paths_out && g->n_paths) || (!pairs_out && cap)) return fail(GFS_E_ARG, "null argument");
    *total = 0;
    int rc = check_diagnosis(z, ratio);
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

// ---------------------------------------------------------------------------------------------
// batches: many configured contexts in one persistent launch (K1f / K2f, sgd_kernels_batch.hip)
// ---------------------------------------------------------------------------------------------
struct BatchLaunch {
    bool lds_tables = false;
    size_t lds_bytes = 0;              // the largest among its items
    uint64_t first = 0, count = 0;     // its items: run[first .. first + count)
    uint64_t blocks = 0, block_offset = 0;   // workgroups; where its part of the block table starts
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct gfs_batch {
    int device = 0, dims = 0;
    uint32_t block = 256;
    std::vector<gfs_ctx *> ctxs;       // as given
    std::vector<uint64_t> run;         // indices into ctxs of the items with something to do, in launch order
    std::vector<BatchLaunch> launches;
    std::vector<uint64_t> pool_offset; // by position in run: first word of the item's counters in d_pool
    std::vector<uint64_t> item_blocks, item_iters;   // by position in run: workgroups and iter_max + 1 as planned at create,
    std::vector<size_t> item_lds;                    // and lds_bytes (0 without LDS tables)
    uint64_t pool_words = 0, total_blocks = 0;
    std::vector<gfs::BatchItem> h_items; std::vector<uint32_t> h_block_item;    // staging of the two tables
    gfs::BatchItem *d_items = nullptr; uint32_t *d_block_item = nullptr; uint32_t *d_pool = nullptr;
    uint64_t launches_done = 0, blocks_done = 0;
    double kernel_ms = 0.0, total_ms = 0.0;
    // K4b / K6b (batch_readout_kernels.hip): the item table, the packed outputs and the per-item sort's scratch, allocated on first use
    uint64_t sort_cap = gfs::SEGMENT_SORT_CAP;       // items of more nodes take K6, one by one (gfs_batch_debug_sort_cap)
    std::vector<gfs::ReadoutItem> h_readout;
    gfs::ReadoutItem *d_readout = nullptr;
    double *d_positions = nullptr; uint32_t *d_order = nullptr; uint64_t packed_cap = 0;
    void *d_sort_tmp = nullptr; uint64_t sort_tmp_bytes = 0;
    void *h_packed = nullptr; uint64_t h_packed_bytes = 0;   // pinned: the two copies land here at full rate, whatever the caller's pages are
    hipEvent_t readout_e0 = nullptr, readout_e1 = nullptr;
    // K4c / K6c and K7g (batch_quality_kernels.hip): one device buffer each, [what the host sends | what the kernels write], grown on demand
    void *d_coords = nullptr; uint64_t coords_bytes = 0;
    void *d_quality = nullptr; uint64_t quality_bytes = 0;
};
// pinned staging of at least `bytes` (what it held is lost)
static int batch_staging(gfs_batch *b, uint64_t bytes) {
    if (b->h_packed_bytes >= bytes) return GFS_OK;
    if (b->h_packed) HIPCHK(hipHostFree(b->h_packed));
    b->h_packed = nullptr; b->h_packed_bytes = 0;
    HIPCHK(hipHostMalloc(&b->h_packed, bytes, hipHostMallocDefault));
    b->h_packed_bytes = bytes;
    return GFS_OK;
}
static int batch_device_buffer(void **d, uint64_t *have, uint64_t bytes) {
    if (*have >= bytes) return GFS_OK;
    if (*d) HIPCHK(hipFree(*d));
    *d = nullptr; *have = 0;
    HIPCHK(hipMalloc(d, bytes));
    *have = bytes;
    return GFS_OK;
}
static_assert(GFS_SEGMENT_SORT_CAP == gfs::SEGMENT_SORT_CAP, "the header's cap is the network's");

static bool batch_item_idle(const gfs_ctx *c) { return !c->valid_paths || c->n_nodes == 0; }
static bool batch_eligible(const gfs_ctx *c) {
    return gfs::batch_eligible(c->shape, c->cfg.trace_per_stream != 0, c->d_its_all != nullptr, batch_item_idle(c));
}

extern "C" {

void gfs_batch_destroy(gfs_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    for (auto &l : b->launches) { if (l.e0) (void)hipEventDestroy(l.e0); if (l.e1) (void)hipEventDestroy(l.e1); }
    if (b->d_items) (void)hipFree(b->d_items);
    if (b->d_block_item) (void)hipFree(b->d_block_item);
    if (b->d_pool) (void)hipFree(b->d_pool);
    if (b->d_readout) (void)hipFree(b->d_readout);
    if (b->d_positions) (void)hipFree(b->d_positions);
    if (b->d_order) (void)hipFree(b->d_order);
    if (b->d_sort_tmp) (void)hipFree(b->d_sort_tmp);
    if (b->h_packed) (void)hipHostFree(b->h_packed);
    if (b->d_coords) (void)hipFree(b->d_coords);
    if (b->d_quality) (void)hipFree(b->d_quality);
    if (b->readout_e0) (void)hipEventDestroy(b->readout_e0);
    if (b->readout_e1) (void)hipEventDestroy(b->readout_e1);
    delete b;
}

int gfs_batch_create(gfs_ctx *const *ctxs, uint64_t n, const gfs_batch_config *cfg, gfs_batch **out) {
    if (!out) return fail(GFS_E_ARG, "out is null");
    *out = nullptr;
    if (!ctxs || n == 0) return fail(GFS_E_ARG, "a batch needs at least one context");
    for (uint64_t i = 0; i < n; ++i) if (!ctxs[i]) return fail(GFS_E_ARG, "batch item " + std::to_string(i) + " is null");
    {
        std::vector<gfs_ctx *> sorted(ctxs, ctxs + n);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) {
            const uint64_t first = (uint64_t)(std::find(ctxs, ctxs + n, *dup) - ctxs);
            const uint64_t second = (uint64_t)(std::find(ctxs + first + 1, ctxs + n, *dup) - ctxs);
            return fail(GFS_E_ARG, "batch item " + std::to_string(second) + " is the same context as item " + std::to_string(first));
        }
    }
    for (uint64_t i = 0; i < n; ++i)
        if (!ctxs[i]->configured) return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": context not set up");
    gfs_batch *b = new (std::nothrow) gfs_batch();
    if (!b) return fail(GFS_E_NOMEM, "out of memory");
    auto refuse = [&](int code, uint64_t i, const std::string &why) {
        delete b;
        return fail(code, "batch item " + std::to_string(i) + ": " + why);
    };
    b->ctxs.assign(ctxs, ctxs + n);
    b->device = ctxs[0]->device; b->dims = ctxs[0]->dims;
    bool have_block = false;
    std::vector<uint64_t> with_lds, without_lds;
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = ctxs[i];
        if (c->device != b->device) return refuse(GFS_E_UNSUPPORTED, i, "on device " + std::to_string(c->device) + ", item 0 on device " + std::to_string(b->device));
        if (c->dims != b->dims)
            return refuse(GFS_E_UNSUPPORTED, i, "dims=" + std::to_string(c->dims) + ", item 0 has dims=" + std::to_string(b->dims) +
                                                    " (a batch is all 1D sorts or all layouts of one dimension)");
        if (batch_item_idle(c)) continue;                                  // counted, not run
        if (!gfs::batch_fused_kernel(c->dims, true))
            return refuse(GFS_E_UNSUPPORTED, i, "no batch kernel is built for dims=" + std::to_string(c->dims) + " (1D sorts, layouts of 2 and 3 dimensions)");
        if (!batch_eligible(c))
            return refuse(GFS_E_UNSUPPORTED, i, "its plan is not the pooled fused reference-stream kernel (bundle=" + std::to_string(c->shape.bundle) +
                                                    " phased=" + std::to_string(c->shape.phased) + " fused=" + std::to_string(c->shape.fused) +
                                                    " trace=" + std::to_string(c->cfg.trace_per_stream != 0) + ")");
        if (c->params.iter_max + 1 > 4096 || c->params.iter_max + 1 == 0)
            return refuse(GFS_E_UNSUPPORTED, i, "iter_max + 1 exceeds the 4096 iterations of one fused launch");
        if (have_block && c->shape.block != b->block)
            return refuse(GFS_E_UNSUPPORTED, i, "block size " + std::to_string(c->shape.block) + ", earlier items have " + std::to_string(b->block));
        b->block = c->shape.block; have_block = true;
        (c->shape.lds_tables ? with_lds : without_lds).push_back(i);
    }
    // ---- device from here on ----
    auto bail = [&](const char *what, hipError_t e) {
        const std::string m = std::string(what) + ": " + hipGetErrorString(e);
        gfs_batch_destroy(b);
        return fail(GFS_E_HIP, m);
    };
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess) return bail("hipSetDevice", e);
    for (const std::vector<uint64_t> *group : {&with_lds, &without_lds}) {
        if (group->empty()) continue;
        const bool lds_tables = group == &with_lds;
        size_t lds_max = 0;
        std::vector<uint64_t> blocks;
        for (uint64_t i : *group) {
            lds_max = std::max(lds_max, ctxs[i]->shape.lds_bytes);
            blocks.push_back((ctxs[i]->shape.n_streams + b->block - 1) / b->block);
        }
        // Every workgroup of a launch is resident at once: a graph whose workgroups start late would walk its early, large-eta
        // iterations after the others have finished theirs (launch_policy.h shape_after_residency has the measurement for the team kernels).
        uint64_t max_blocks = cfg ? cfg->max_blocks_per_launch : 0;
        if (!max_blocks) {
            int per_cu = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gfs::batch_fused_kernel(b->dims, lds_tables), (int)b->block, lds_max);
            if (e != hipSuccess) return bail("hipOccupancyMaxActiveBlocksPerMultiprocessor", e);
            max_blocks = (uint64_t)std::max(per_cu, 0) * (uint64_t)ctxs[0]->cu_count;
        }
        max_blocks = std::min<uint64_t>(max_blocks, 0x7FFFFFFFull);        // a grid's x dimension
        std::vector<uint32_t> launch_of(blocks.size());
        uint32_t n_launches = 0;
        const uint64_t bad = gfs::batch_plan(blocks.data(), blocks.size(), max_blocks, launch_of.data(), &n_launches);
        if (bad < blocks.size()) {
            const uint64_t i = (*group)[bad];
            const std::string why = "its " + std::to_string(blocks[bad]) + " workgroups exceed the " + std::to_string(max_blocks) + " one launch may hold";
            gfs_batch_destroy(b);
            return fail(GFS_E_UNSUPPORTED, "batch item " + std::to_string(i) + ": " + why);
        }
        const size_t base = b->launches.size();
        b->launches.resize(base + n_launches);
        for (size_t k = 0; k < blocks.size(); ++k) {
            BatchLaunch &l = b->launches[base + launch_of[k]];
            if (l.count == 0) { l.first = b->run.size(); l.lds_tables = lds_tables; l.block_offset = b->total_blocks; }
            l.count++; l.blocks += blocks[k];
            if (lds_tables) l.lds_bytes = std::max(l.lds_bytes, ctxs[(*group)[k]]->shape.lds_bytes);
            b->run.push_back((*group)[k]);
            b->pool_offset.push_back(b->pool_words);
            b->item_blocks.push_back(blocks[k]);
            b->item_iters.push_back(ctxs[(*group)[k]]->params.iter_max + 1);
            b->item_lds.push_back(lds_tables ? ctxs[(*group)[k]]->shape.lds_bytes : 0);
            b->pool_words += gfs::pool_bytes(ctxs[(*group)[k]]->params.iter_max + 1) / sizeof(uint32_t);
            b->total_blocks += blocks[k];
        }
    }
    if (!b->run.empty()) {
        b->h_items.resize(b->run.size());
        b->h_block_item.resize(b->total_blocks);
        if ((e = hipMalloc(&b->d_items, b->run.size() * sizeof(gfs::BatchItem))) != hipSuccess) return bail("hipMalloc items", e);
        if ((e = hipMalloc(&b->d_block_item, b->total_blocks * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc block table", e);
        if ((e = hipMalloc(&b->d_pool, b->pool_words * sizeof(uint32_t))) != hipSuccess) return bail("hipMalloc pools", e);
        for (auto &l : b->launches) {
            if ((e = hipEventCreate(&l.e0)) != hipSuccess || (e = hipEventCreate(&l.e1)) != hipSuccess) return bail("hipEventCreate", e);
        }
    }
    *out = b;
    return GFS_OK;
}

int gfs_batch_run(gfs_batch *b, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    for (size_t i = 0; i < b->ctxs.size(); ++i)
        if (!b->ctxs[i]->configured) return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": context not set up");
    if (b->run.empty()) return GFS_NOTHING_TO_DO;
    // the launches, the block table and the pools were sized at create: a context set up again since then no longer fits them
    for (size_t r = 0; r < b->run.size(); ++r) {
        const gfs_ctx *c = b->ctxs[b->run[r]];
        const bool same_plan = c->dims == b->dims && c->shape.block == b->block && batch_eligible(c) &&
                               (c->shape.lds_tables ? c->shape.lds_bytes : 0) == b->item_lds[r];
        if (!same_plan || (c->shape.n_streams + b->block - 1) / b->block != b->item_blocks[r] || c->params.iter_max + 1 != b->item_iters[r])
            return fail(GFS_E_STATE, "batch item " + std::to_string(b->run[r]) + ": set up again since the batch was created (" +
                                         std::to_string(c->shape.n_streams) + " streams, iter_max " + std::to_string(c->params.iter_max) + ")");
    }
    auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // the two tables, from the contexts as they are now (positions may have been bound anew since the last run)
    for (const BatchLaunch &l : b->launches) {
        uint64_t block = 0;
        for (uint64_t r = l.first; r < l.first + l.count; ++r) {
            const gfs_ctx *c = b->ctxs[b->run[r]];
            gfs::BatchItem &it = b->h_items[r];
            it = gfs::BatchItem{};
            fill_kargs(c, it.a);
            it.a.it = iter_consts(c, 0);
            it.its = c->d_its_all;
            it.pool = b->d_pool + b->pool_offset[r];
            it.n_iters = (uint32_t)(c->params.iter_max + 1);
            it.first_block = (uint32_t)block;
            const uint64_t nb = b->item_blocks[r];
            for (uint64_t k = 0; k < nb; ++k) b->h_block_item[l.block_offset + block + k] = (uint32_t)r;
            block += nb;
        }
    }
    HIPCHK(hipMemcpyAsync(b->d_items, b->h_items.data(), b->h_items.size() * sizeof(gfs::BatchItem), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_block_item, b->h_block_item.data(), b->h_block_item.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // work pools (sgd_kernel_common.h pool_walk): every item's counters, zeroed per run
    HIPCHK(hipMemsetAsync(b->d_pool, 0, b->pool_words * sizeof(uint32_t), st));
    for (BatchLaunch &l : b->launches) {
        const gfs::BatchItem *items = b->d_items;
        const uint32_t *block_item = b->d_block_item + l.block_offset;
        void *args[] = {&items, &block_item};
        HIPCHK(hipEventRecord(l.e0, st));                  // (the event pair brackets the kernel alone)
        hipError_t e = hipLaunchKernel(gfs::batch_fused_kernel(b->dims, l.lds_tables), dim3((unsigned)l.blocks), dim3(b->block), args, l.lds_bytes, st);
        if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch kernel launch: ") + hipGetErrorString(e));
        HIPCHK(hipEventRecord(l.e1, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (BatchLaunch &l : b->launches) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, l.e0, l.e1) == hipSuccess) b->kernel_ms += t;
        b->launches_done++; b->blocks_done += l.blocks;
    }
    for (uint64_t r : b->run) {                            // each context as if it had been run alone (its kernel_ms apart)
        gfs_ctx *c = b->ctxs[r];
        c->iterations += c->params.iter_max + 1;
        c->launches++;
    }
    b->total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GFS_OK;
}

int gfs_batch_get_stats(gfs_batch *b, gfs_batch_stats *out) {
    if (!b || !out) return fail(GFS_E_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    out->items = b->ctxs.size(); out->items_run = b->run.size();
    out->launches = b->launches_done; out->blocks = b->blocks_done;
    out->kernel_ms = b->kernel_ms; out->total_ms = b->total_ms;
    for (uint64_t r : b->run) {
        gfs_stats st;
        int rc = gfs_ctx_stats(b->ctxs[r], &st);
        if (rc) return rc;
        out->term_updates += st.term_updates; out->attempts += st.attempts;
    }
    return GFS_OK;
}

// ---- K4b / K6b: every item's start positions, and every item's positions and rank order, in one launch ------------------------
static uint64_t batch_total_nodes(const gfs_batch *b) {
    uint64_t total = 0;
    for (const gfs_ctx *c : b->ctxs) total += c->n_nodes;
    return total;
}
// the checks gfs_ctx_init_positions and gfs_ctx_sort_order make, on every item; no device call
static int batch_readout_check(const gfs_batch *b) {
    if (b->dims != 0) return fail(GFS_E_UNSUPPORTED, "a batch of layouts has no start positions or rank order (dims=" + std::to_string(b->dims) +
                                                          "): use gfs_batch_upload_coords and gfs_batch_coords");
    for (size_t i = 0; i < b->ctxs.size(); ++i) {
        const gfs_ctx *c = b->ctxs[i];
        if (!c->d_x || c->dims != 0) return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": needs a 1D context that has been set up");
    }
    return GFS_OK;
}
// The item table from the contexts as they are now (positions may have been bound anew), in the order `order` lists them;
// offsets are those of gfs_batch_result_offsets.  Uploaded on st.
static int batch_readout_table(gfs_batch *b, const std::vector<uint64_t> &order, hipStream_t st) {
    if (!b->d_readout) HIPCHK(hipMalloc(&b->d_readout, b->ctxs.size() * sizeof(gfs::ReadoutItem)));
    std::vector<uint64_t> offset(b->ctxs.size());
    uint64_t total = 0;
    for (size_t i = 0; i < b->ctxs.size(); ++i) { offset[i] = total; total += b->ctxs[i]->n_nodes; }
    b->h_readout.resize(order.size());
    for (size_t r = 0; r < order.size(); ++r) {
        const gfs_ctx *c = b->ctxs[order[r]];
        gfs::ReadoutItem &it = b->h_readout[r];
        it.x = c->d_x; it.perm = c->d_perm; it.node_len = c->d_node_len;
        it.offset = offset[order[r]];
        it.n = (uint32_t)c->n_nodes;                                       // (a context has fewer than 2^31 nodes)
        it.padded = c->n_nodes <= gfs::SEGMENT_SORT_CAP ? gfs::segment_padded(it.n) : 0;
    }
    if (!order.empty())
        HIPCHK(hipMemcpyAsync(b->d_readout, b->h_readout.data(), order.size() * sizeof(gfs::ReadoutItem), hipMemcpyHostToDevice, st));
    return GFS_OK;
}

int gfs_batch_result_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n) {
    if (!b || !offsets) return fail(GFS_E_ARG, "null argument");
    if (n != b->ctxs.size() + 1) return fail(GFS_E_ARG, "offsets: need items + 1 entries");
    uint64_t total = 0;
    for (size_t i = 0; i < b->ctxs.size(); ++i) { offsets[i] = total; total += b->ctxs[i]->n_nodes; }
    offsets[b->ctxs.size()] = total;
    return GFS_OK;
}

int gfs_batch_debug_sort_cap(gfs_batch *b, uint64_t cap) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    if (cap > gfs::SEGMENT_SORT_CAP) return fail(GFS_E_ARG, "sort cap above GFS_SEGMENT_SORT_CAP");
    b->sort_cap = cap ? cap : gfs::SEGMENT_SORT_CAP;
    return GFS_OK;
}

int gfs_batch_init_positions(gfs_batch *b, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    int rc = batch_readout_check(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_init_positions: nothing of an item is in flight
    hipStream_t st = (hipStream_t)hip_stream;
    std::vector<uint64_t> all(b->ctxs.size());
    std::iota(all.begin(), all.end(), 0ull);
    rc = batch_readout_table(b, all, st);
    if (rc) return rc;
    hipError_t e = gfs::batch_init_positions_device(b->d_readout, (uint32_t)all.size(), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch init_positions: ") + hipGetErrorString(e));
    HIPCHK(hipStreamSynchronize(st));
    return GFS_OK;
}

int gfs_batch_results(gfs_batch *b, double *positions, uint32_t *order, uint64_t total, double *kernel_ms, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    if (!positions && !order) return fail(GFS_E_ARG, "both output buffers are null");
    if (total != batch_total_nodes(b)) return fail(GFS_E_ARG, "total is not the batch's node count (gfs_batch_result_offsets)");
    int rc = batch_readout_check(b);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_sort_order
    hipStream_t st = (hipStream_t)hip_stream;
    if (b->packed_cap < total) {
        if (b->d_positions) HIPCHK(hipFree(b->d_positions));
        if (b->d_order) HIPCHK(hipFree(b->d_order));
        b->d_positions = nullptr; b->d_order = nullptr; b->packed_cap = 0;
        HIPCHK(hipMalloc(&b->d_positions, total * sizeof(double)));
        HIPCHK(hipMalloc(&b->d_order, total * sizeof(uint32_t)));
        b->packed_cap = total;
    }
    if (!b->readout_e0) HIPCHK(hipEventCreate(&b->readout_e0));
    if (!b->readout_e1) HIPCHK(hipEventCreate(&b->readout_e1));
    // items within the cap by the length of their padded segment: one launch per length, its LDS and block sized by it; the others after them
    std::vector<uint64_t> by_len(b->ctxs.size());
    std::iota(by_len.begin(), by_len.end(), 0ull);
    auto padded_of = [&](uint64_t i) -> uint64_t {
        const uint64_t n = b->ctxs[i]->n_nodes;
        return n <= b->sort_cap ? gfs::segment_padded((uint32_t)n) : ~0ull;
    };
    std::stable_sort(by_len.begin(), by_len.end(), [&](uint64_t a, uint64_t c) { return padded_of(a) < padded_of(c); });
    rc = batch_readout_table(b, by_len, st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(b->readout_e0, st));
    size_t first = 0;
    while (first < by_len.size() && padded_of(by_len[first]) != ~0ull) {
        const uint64_t P = padded_of(by_len[first]);
        size_t end = first;
        while (end < by_len.size() && padded_of(by_len[end]) == P) ++end;
        for (size_t at = first; at < end; at += 0x7FFFFFFFull) {           // (a grid's x dimension)
            const uint32_t count = (uint32_t)std::min<size_t>(end - at, 0x7FFFFFFFull);
            hipError_t e = gfs::sort_segments_device(b->d_readout + at, count, (uint32_t)P, positions ? b->d_positions : nullptr, b->d_order, st);
            if (e != hipSuccess) return fail(GFS_E_HIP, std::string("segment sort launch: ") + hipGetErrorString(e));
        }
        first = end;
    }
    // above the cap: K6 (rocPRIM radix sort) once each, into the same packed arrays
    for (size_t r = first; r < by_len.size(); ++r) {
        const gfs_ctx *c = b->ctxs[by_len[r]];
        const gfs::ReadoutItem &it = b->h_readout[r];
        const uint64_t n = c->n_nodes, need = n * (2 * 8 + 2 * 4);
        HIPCHK(hipStreamSynchronize(st));                                  // (K6 runs on the null stream)
        if (b->sort_tmp_bytes < need) {
            if (b->d_sort_tmp) HIPCHK(hipFree(b->d_sort_tmp));
            b->d_sort_tmp = nullptr; b->sort_tmp_bytes = 0;
            HIPCHK(hipMalloc(&b->d_sort_tmp, need));
            b->sort_tmp_bytes = need;
        }
        uint32_t *d_sorted = nullptr;
        hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, b->d_sort_tmp, &d_sorted);
        if (e != hipSuccess) return fail(GFS_E_HIP, "batch item " + std::to_string(by_len[r]) + ": sort_order_device: " + hipGetErrorString(e));
        HIPCHK(hipMemcpyAsync(b->d_order + it.offset, d_sorted, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (positions) {
            e = gfs::reorder_positions_device(c->d_x, b->d_positions + it.offset, c->d_perm, n, 0, 0, st);
            if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch positions: ") + hipGetErrorString(e));
        }
        HIPCHK(hipStreamSynchronize(st));                                  // (the scratch is the next item's)
    }
    HIPCHK(hipEventRecord(b->readout_e1, st));
    // The two copies go through pinned memory of the batch: a copy of megabytes straight into the caller's pageable buffer has
    // the runtime pin those pages first, 20-30 ms where they are fresh (profiles/r10/batch_readout_probe_pageable.log).
    const uint64_t staging = total * (sizeof(double) + sizeof(uint32_t));
    if (b->h_packed_bytes < staging) {
        if (b->h_packed) HIPCHK(hipHostFree(b->h_packed));
        b->h_packed = nullptr; b->h_packed_bytes = 0;
        HIPCHK(hipHostMalloc(&b->h_packed, staging, hipHostMallocDefault));
        b->h_packed_bytes = staging;
    }
    double *h_positions = reinterpret_cast<double *>(b->h_packed);
    uint32_t *h_order = reinterpret_cast<uint32_t *>(h_positions + total);
    if (positions && total) HIPCHK(hipMemcpyAsync(h_positions, b->d_positions, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (order && total) HIPCHK(hipMemcpyAsync(h_order, b->d_order, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (positions && total) std::memcpy(positions, h_positions, total * sizeof(double));
    if (order && total) std::memcpy(order, h_order, total * sizeof(uint32_t));
    float t = 0.f;
    if (kernel_ms && hipEventElapsedTime(&t, b->readout_e0, b->readout_e1) == hipSuccess) *kernel_ms = t;
    return GFS_OK;
}

// ---- K4c / K6c: every item's layout coordinates, up or down, in one launch and one copy of coordinates -------------------------
// The checks of both directions, on every item; no device call.  *total_out = the packed length in doubles.
static int batch_coords_check(const gfs_batch *b, const double *coords, uint64_t total) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    if (!coords) return fail(GFS_E_ARG, "coords is null");
    if (b->dims == 0)
        return fail(GFS_E_UNSUPPORTED, "a batch of 1D sorts has no layout coordinates: use gfs_batch_init_positions and gfs_batch_results");
    uint64_t want = 0;
    for (size_t i = 0; i < b->ctxs.size(); ++i) {
        const gfs_ctx *c = b->ctxs[i];
        if (c->dims != b->dims || c->x_len != c->n_nodes * 2 * (uint64_t)b->dims || (c->x_len && !c->d_x))
            return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": needs a context set up for layouts of " + std::to_string(b->dims) + " dimensions");
        want += c->x_len;
    }
    if (total != want) return fail(GFS_E_ARG, "total is not the batch's node count * 2 * dimensions (gfs_batch_result_offsets)");
    return GFS_OK;
}
// One call either way.  Device buffer and pinned staging: [packed coordinates | CoordItem table | block table]; up, the whole of it
// goes in one copy; down, the two tables go up and the coordinates come back.
static int batch_coords_move(gfs_batch *b, double *coords, uint64_t total, int to_device, double *kernel_ms, hipStream_t st) {
    if (kernel_ms) *kernel_ms = 0.0;
    const uint64_t n = b->ctxs.size();
    std::vector<uint64_t> nodes(n), word_offset(n + 1), first_block(n + 1);
    for (uint64_t i = 0; i < n; ++i) nodes[i] = b->ctxs[i]->n_nodes;
    const uint64_t blocks = gfs::coord_plan(nodes.data(), n, (uint32_t)b->dims, word_offset.data(), first_block.data());
    if (blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's coordinates exceed one launch");
    if (total == 0) return GFS_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_download_positions: nothing of an item is in flight
    const uint64_t tables_at = total * sizeof(double), blocks_at = tables_at + n * sizeof(gfs::CoordItem);
    const uint64_t bytes = blocks_at + blocks * sizeof(uint32_t);
    int rc = batch_staging(b, bytes);
    if (!rc) rc = batch_device_buffer(&b->d_coords, &b->coords_bytes, bytes);
    if (rc) return rc;
    if (!b->readout_e0) HIPCHK(hipEventCreate(&b->readout_e0));
    if (!b->readout_e1) HIPCHK(hipEventCreate(&b->readout_e1));
    unsigned char *h = reinterpret_cast<unsigned char *>(b->h_packed), *d = reinterpret_cast<unsigned char *>(b->d_coords);
    gfs::CoordItem *h_items = reinterpret_cast<gfs::CoordItem *>(h + tables_at);
    for (uint64_t i = 0; i < n; ++i) {                                     // from the contexts as they are now (positions may have been bound anew)
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::CoordItem{c->d_x, c->d_perm, word_offset[i], (uint32_t)c->n_nodes, (uint32_t)first_block[i], (uint32_t)b->dims, 0u};
    }
    gfs::block_item_table(first_block.data(), n, reinterpret_cast<uint32_t *>(h + blocks_at));
    if (to_device) {
        std::memcpy(h, coords, total * sizeof(double));
        HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(d + tables_at, h + tables_at, bytes - tables_at, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipEventRecord(b->readout_e0, st));
    hipError_t e = gfs::batch_coords_device(reinterpret_cast<const gfs::CoordItem *>(d + tables_at), reinterpret_cast<const uint32_t *>(d + blocks_at),
                                            blocks, reinterpret_cast<double *>(d), to_device, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch coordinates launch: ") + hipGetErrorString(e));
    HIPCHK(hipEventRecord(b->readout_e1, st));
    if (!to_device) HIPCHK(hipMemcpyAsync(h, d, total * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!to_device) std::memcpy(coords, h, total * sizeof(double));
    float t = 0.f;
    if (kernel_ms && hipEventElapsedTime(&t, b->readout_e0, b->readout_e1) == hipSuccess) *kernel_ms = t;
    return GFS_OK;
}

int gfs_batch_upload_coords(gfs_batch *b, const double *coords, uint64_t total, void *hip_stream) {
    int rc = batch_coords_check(b, coords, total);
    if (rc) return rc;
    return batch_coords_move(b, const_cast<double *>(coords), total, 1, nullptr, (hipStream_t)hip_stream);
}

int gfs_batch_coords(gfs_batch *b, double *coords, uint64_t total, double *kernel_ms, void *hip_stream) {
    int rc = batch_coords_check(b, coords, total);
    if (rc) return rc;
    return batch_coords_move(b, coords, total, 0, kernel_ms, (hipStream_t)hip_stream);
}

// ---- K7g: gfs_ctx_pair_errors of every item, sorts and layouts alike, in one step launch and one reduce launch --------------------
int gfs_batch_pair_errors(gfs_batch *b, const uint64_t *zs, uint64_t n_z, gfs_pair_error *out, double *kernel_ms, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    int rc = check_step_distances(zs, n_z, out);
    if (rc) return rc;
    const uint64_t n = b->ctxs.size();
    for (uint64_t i = 0; i < n; ++i)
        if (!b->ctxs[i]->d_x || b->ctxs[i]->dims != b->dims)
            return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": the context has no positions (not set up)");
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_z == 0) return GFS_OK;
    std::vector<uint64_t> steps(n), first_block(n + 1);
    for (uint64_t i = 0; i < n; ++i) steps[i] = b->ctxs[i]->n_steps;
    const uint64_t row_blocks = gfs::quality_plan(steps.data(), n, first_block.data());
    if (row_blocks > 0x7FFFFFFFull || n > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's step tables exceed one launch");
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // device: [zs | QualityItem table | block table (whole words) | out words | partials]; the first three go up in one copy
    const uint64_t items_at = n_z * 8, blocks_at = items_at + n * sizeof(gfs::QualityItem);
    const uint64_t out_at = blocks_at + (row_blocks * sizeof(uint32_t) + 7) / 8 * 8, out_bytes = n * n_z * 5 * 8;
    const uint64_t partials_at = out_at + out_bytes, bytes = partials_at + 5 * n_z * row_blocks * 8;
    rc = batch_staging(b, out_at + out_bytes);                             // (staging: the same offsets, less the partials)
    if (!rc) rc = batch_device_buffer(&b->d_quality, &b->quality_bytes, bytes);
    if (rc) return rc;
    if (!b->readout_e0) HIPCHK(hipEventCreate(&b->readout_e0));
    if (!b->readout_e1) HIPCHK(hipEventCreate(&b->readout_e1));
    unsigned char *h = reinterpret_cast<unsigned char *>(b->h_packed), *d = reinterpret_cast<unsigned char *>(b->d_quality);
    std::memcpy(h, zs, n_z * 8);
    gfs::QualityItem *h_items = reinterpret_cast<gfs::QualityItem *>(h + items_at);
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::QualityItem{c->d_step_rec, c->d_x, c->n_steps, c->n_nodes, (uint32_t)first_block[i], (uint32_t)(first_block[i + 1] - first_block[i])};
    }
    gfs::block_item_table(first_block.data(), n, reinterpret_cast<uint32_t *>(h + blocks_at));
    HIPCHK(hipMemcpyAsync(d, h, blocks_at + row_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(b->readout_e0, st));
    hipError_t e = gfs::batch_pair_errors_device(reinterpret_cast<const gfs::QualityItem *>(d + items_at), reinterpret_cast<const uint32_t *>(d + blocks_at),
                                                 (uint32_t)n, row_blocks, (uint32_t)b->dims, reinterpret_cast<const uint64_t *>(d), (uint32_t)n_z,
                                                 reinterpret_cast<uint64_t *>(d + partials_at), reinterpret_cast<uint64_t *>(d + out_at), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch pair_errors launch: ") + hipGetErrorString(e));
    HIPCHK(hipEventRecord(b->readout_e1, st));
    HIPCHK(hipMemcpyAsync(h + out_at, d + out_at, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t *w = reinterpret_cast<const uint64_t *>(h + out_at);
    for (uint64_t r = 0; r < n * n_z; ++r) {
        gfs_pair_error &o = out[r];
        o.step_distance = zs[r % n_z]; o.pairs = w[5 * r];
        std::memcpy(&o.sum_rel_sq, &w[5 * r + 1], 8); std::memcpy(&o.max_rel_sq, &w[5 * r + 2], 8);
        std::memcpy(&o.sum_abs, &w[5 * r + 3], 8); std::memcpy(&o.sum_sq, &w[5 * r + 4], 8);
    }
    float t = 0.f;
    if (kernel_ms && hipEventElapsedTime(&t, b->readout_e0, b->readout_e1) == hipSuccess) *kernel_ms = t;
    return GFS_OK;
}

}  // extern "C"
