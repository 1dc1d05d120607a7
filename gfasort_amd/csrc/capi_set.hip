// capi_set.hip — the context sets of the C ABI (include/gfasort_hip.h, gfs_ctx_set_*): many gfs_ctx (capi.hip, capi_ctx.h) built
// from many graph views in ONE pass over their disjoint union (K3b, index_set_kernels.hip), and the driver of that build, which
// gfs_ctx_create shares: a single context is a set of one.  The items' index arrays live in one arena the set owns, the items
// borrow them.  gfs_ctx_set_setup_* sets every item up in one pass (K3c, set_setup_kernels.hip), their state arrays in a second
// arena of the set's; the driver of that setup is here too, and gfs_ctx_setup_* shares it: again a set of one, with an arena of the
// context's own.
#include "capi_ctx.h"
#include "index_set.h"
#include "set_seed_tables.h"
#include "set_state_plan.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>

struct gfs_ctx_set {
    int device = 0;
    gfs::Buffer arena;                              // every item's step records, path records, path lengths, node layout, node lengths
    gfs::Buffer state_arena;                        // gfs_ctx_set_setup_*: every item's state arrays, the seeding kernel's tables behind them
    gfs::Buffer h_stage{true};                      // ... and the pinned staging of what a set setup sends up; both kept between setups
    std::vector<std::unique_ptr<gfs_ctx>> items;    // (declared after the arenas: they go first)
    gfs_ctx_set_info info{};
    gfs_ctx_set_setup_info setup_info{};
};

namespace {
constexpr int KINDS = gfs::SET_KINDS;
std::string item_prefix(uint64_t i) { return "set item " + std::to_string(i) + ": "; }
}  // namespace

// (capi_ctx.h says what the parameters mean)
int gfs::build_contexts(const gfs_graph_view *const *graphs, gfs_ctx *const *ctxs, uint64_t n, gfs::Buffer &arena, const uint32_t *node_perm,
                        bool staged, gfs::Laps *laps, gfs_ctx_set_info *info) {
    const std::string set = staged ? "set " : "";
    auto lap = [laps](const char *what) { if (laps && laps->on) { (void)hipDeviceSynchronize(); laps->lap(what); } };
    int rc = GFS_OK;
    auto ok = [&rc, &set](const char *call, const char *what, hipError_t err) {   // false: rc holds the reported error
        if (err != hipSuccess) rc = fail(GFS_E_HIP, std::string(call) + " " + set + what + ": " + hipGetErrorString(err));
        return err == hipSuccess;
    };
    std::vector<uint64_t> counts(3 * n), offsets(KINDS * n);
    uint64_t N = 0, S = 0, P = 0;
    for (uint64_t i = 0; i < n; ++i) {
        counts[i] = ctxs[i]->n_nodes; counts[n + i] = ctxs[i]->n_steps; counts[2 * n + i] = ctxs[i]->n_paths;
        N += ctxs[i]->n_nodes; S += ctxs[i]->n_steps; P += ctxs[i]->n_paths;
    }
    const uint64_t arena_bytes = gfs::set_arena_plan(counts.data(), counts.data() + n, counts.data() + 2 * n, n, offsets.data());
    const uint64_t perm_begin = offsets[3], nlen_begin = offsets[4];      // (by kind: the layouts end where the node lengths begin)
    const uint64_t perm_bytes = nlen_begin - perm_begin, nlen_bytes = arena_bytes - nlen_begin;

    // the input head of the device scratch: [step_node | path_first | item table | step_is_rev].  A set gathers it in pinned staging
    // and sends it up in one copy, the node lengths from the staging's tail straight to their range of the arena, and the layouts
    // come back into the staging; a single graph's arrays are the head's parts as they are, and go up one by one.
    const gfs::SetInputHead in = gfs::set_input_head(S, P, n);
    uint64_t work_bytes = 0;
    hipError_t e = gfs::index_set_work_bytes(N, S, &work_bytes);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("rocPRIM temporary storage: ") + hipGetErrorString(e));
    gfs::Buffer h_stage{true}, d_scratch;                                  // (freed after the synchronise that ends the build)
    if ((rc = arena.reserve(std::max<uint64_t>(arena_bytes, 256), ("hipMalloc " + set + "arena").c_str()))) return rc;
    if ((rc = d_scratch.reserve(in.bytes + work_bytes, ("hipMalloc " + set + "scratch").c_str()))) return rc;
    if (staged && (rc = h_stage.reserve(std::max(in.bytes + nlen_bytes, perm_bytes), "hipHostMalloc set staging"))) return rc;
    info->device_allocations = staged ? 3 : 2;
    if (!ok("hipMemset", "arena", hipMemsetAsync(arena.p, 0, std::max<uint64_t>(arena_bytes, 256), 0))) return rc;
    ++info->launches;

    std::vector<gfs::SetItem> items(n + 1);
    uint64_t node_off = 0, step_off = 0, path_off = 0;
    for (uint64_t i = 0; i <= n; ++i) {
        items[i] = gfs::SetItem{node_off, step_off, path_off, 0, 0, 0, 0, 0};
        if (i == n) break;
        const uint64_t *at = &offsets[KINDS * i];
        items[i].rec = at[0]; items[i].prec = at[1]; items[i].plen = at[2]; items[i].perm = at[3]; items[i].nlen = at[4];
        node_off += ctxs[i]->n_nodes; step_off += ctxs[i]->n_steps; path_off += ctxs[i]->n_paths;
    }
    unsigned char *h = h_stage.as<unsigned char>(), *d_in = d_scratch.as<unsigned char>(), *d_arena = arena.as<unsigned char>();
    if (staged) {
        auto *h_step_node = reinterpret_cast<uint32_t *>(h);
        auto *h_first = reinterpret_cast<uint64_t *>(h + in.at_first);
        uint8_t *h_rev = h + in.at_rev;
        unsigned char *h_nlen = h + in.bytes;
        std::memset(h_nlen, 0, nlen_bytes);
        for (uint64_t i = 0; i < n; ++i) {
            const gfs_graph_view *g = graphs[i];
            const gfs::SetItem &it = items[i];
            if (g->n_steps) {
                std::memcpy(h_step_node + it.step_off, g->step_node, g->n_steps * 4);
                std::memcpy(h_rev + it.step_off, g->step_is_rev, g->n_steps);
            }
            for (uint64_t p = 0; p < g->n_paths; ++p) h_first[it.path_off + p] = it.step_off + g->path_first_step[p];
            if (g->n_nodes) std::memcpy(h_nlen + (it.nlen - nlen_begin), g->node_len, g->n_nodes * 4);
        }
        h_first[P] = S;
        std::memcpy(h + in.at_items, items.data(), items.size() * sizeof(gfs::SetItem));
        if (!ok("hipMemcpy", "inputs", hipMemcpyAsync(d_in, h, in.bytes, hipMemcpyHostToDevice, 0))) return rc;
        if (nlen_bytes && !ok("hipMemcpy", "node_len", hipMemcpyAsync(d_arena + nlen_begin, h_nlen, nlen_bytes, hipMemcpyHostToDevice, 0))) return rc;
    } else {
        const gfs_graph_view *g = graphs[0];                               // (its first steps are union steps as they are)
        if (N && !ok("hipMemcpy", "node_len", hipMemcpy(d_arena + nlen_begin, g->node_len, N * 4, hipMemcpyHostToDevice))) return rc;
        if (S && !ok("hipMemcpy", "step_node", hipMemcpy(d_in, g->step_node, S * 4, hipMemcpyHostToDevice))) return rc;
        if (!ok("hipMemcpy", "path_first", hipMemcpy(d_in + in.at_first, g->path_first_step, (P + 1) * 8, hipMemcpyHostToDevice))) return rc;
        if (!ok("hipMemcpy", "item table", hipMemcpy(d_in + in.at_items, items.data(), items.size() * sizeof(gfs::SetItem), hipMemcpyHostToDevice))) return rc;
        if (S && !ok("hipMemcpy", "step_is_rev", hipMemcpy(d_in + in.at_rev, g->step_is_rev, S, hipMemcpyHostToDevice))) return rc;
        if (N && node_perm && !ok("hipMemcpy", "perm", hipMemcpy(d_arena + perm_begin, ctxs[0]->perm.data(), N * 4, hipMemcpyHostToDevice))) return rc;
    }
    lap("step upload");

    gfs::SetUnion u{};
    u.n_items = (uint32_t)n; u.n_nodes = N; u.n_steps = S; u.n_paths = P;
    u.step_node = reinterpret_cast<const uint32_t *>(d_in);
    u.path_first = reinterpret_cast<const uint64_t *>(d_in + in.at_first);
    u.items = reinterpret_cast<const gfs::SetItem *>(d_in + in.at_items);
    u.step_is_rev = d_in + in.at_rev;
    u.arena = d_arena;
    // A single context: 8-byte trip records beside the step records, written by the same pass (sgd_1d.h TripRec), and the facts that
    // say whether its trips may read them (launch_policy.h compact_records).  Its launch shape is not known before its setup, so the
    // array is made here for every graph with steps and given back at once where a position does not fit its 32 bits or a node
    // repeats within 64 steps (b > 0), and by a layout's setup (setup_contexts); an allocation that fails is no error: the
    // context keeps full records.
    gfs_ctx *single = staged || n != 1 ? nullptr : ctxs[0];
    if (single && S && single->d_trip_rec.grow((S + 1) * sizeof(uint2)) != hipSuccess) (void)hipGetLastError();
    u.trip = single ? (uint2 *)single->d_trip_rec : nullptr;
    uint32_t bad_item = gfs::SET_NO_BAD_ITEM;
    e = gfs::index_set_layout_device(u, d_in + in.bytes, node_perm != nullptr, &bad_item, &info->launches);
    lap("node layout");
    if (e == hipSuccess && bad_item == gfs::SET_NO_BAD_ITEM)
        e = gfs::index_set_records_device(u, d_in + in.bytes, &info->launches, single ? &single->record_facts : nullptr);
    if (e != hipSuccess || bad_item != gfs::SET_NO_BAD_ITEM) (void)hipDeviceSynchronize();   // (nothing in flight when the buffers go)
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("build_index_set: ") + hipGetErrorString(e));
    if (bad_item != gfs::SET_NO_BAD_ITEM) return fail(GFS_E_ARG, (staged ? item_prefix(bad_item) : "") + "step_node out of range");
    // every layout back in one copy (blocking: it ends the build): a set's into the staging, a single context's into its perm —
    // unless that holds the caller's own
    if (staged) {
        if (!ok("hipMemcpy", "perm", hipMemcpy(h, d_arena + perm_begin, std::max<uint64_t>(perm_bytes, 4), hipMemcpyDeviceToHost))) return rc;
    } else if (N && !node_perm) {
        if (!ok("hipMemcpy", "perm", hipMemcpy(ctxs[0]->perm.data(), d_arena + perm_begin, N * 4, hipMemcpyDeviceToHost))) return rc;
    }
    if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(GFS_E_HIP, std::string("hipDeviceSynchronize: ") + hipGetErrorString(e));
    lap("K3");
    if (single) {
        // no onset makes such a graph eligible (launch_policy.h compact_records): a position past 32 bits, a tandem repeat
        if (single->record_facts.max_pos >= (1ull << 32) || single->record_facts.max_b > 0) single->d_trip_rec.reset();
        single->record_facts.have_trip_rec = single->d_trip_rec != nullptr;
    }
    for (uint64_t i = 0; i < n; ++i) {
        gfs_ctx *c = ctxs[i];
        const uint64_t *at = &offsets[KINDS * i];
        if (staged) {
            const uint32_t *perm = reinterpret_cast<const uint32_t *>(h + (at[3] - perm_begin));
            c->perm.assign(perm, perm + c->n_nodes);
        }
        (void)c->d_step_rec.borrow(d_arena + at[0]);
        (void)c->d_path_rec.borrow(d_arena + at[1]);
        (void)c->d_path_len.borrow(d_arena + at[2]);
        (void)c->d_perm.borrow(d_arena + at[3]);
        (void)c->d_node_len.borrow(d_arena + at[4]);
    }
    info->items = n; info->total_nodes = N; info->total_steps = S; info->total_paths = P;
    info->arena_bytes = arena_bytes;
    return GFS_OK;
}

// ---- setup (K3c) -----------------------------------------------------------------------------------------------------------------
// (capi_ctx.h says what the parameters mean)
int gfs::setup_contexts(gfs_ctx *const *ctxs, const gfs_sgd_params *const *params, const int *dims, const gfs_launch_config *cfgs, uint64_t n,
                        gfs::Buffer &arena, gfs::Buffer *pinned, const double *etas, const double *zetas, int32_t *item_rc,
                        gfs_ctx_set_setup_info *info_out) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool single = pinned == nullptr;
    const std::string set = single ? "" : "set ";
    auto named = [single](uint64_t i, const std::string &text) { return single ? text : item_prefix(i) + text; };
    std::string err;
    for (uint64_t i = 0; i < n; ++i) {                                     // (no item is touched, no device call is made, before all pass)
        if (dims[i] < 0) return fail(GFS_E_UNSUPPORTED, named(i, "dimensions must be 1..8"));   // as gfs_ctx_setup_nd: before its other arguments
        if (int rc = gfs::check_setup_args(params[i], dims[i], cfgs ? &cfgs[i] : nullptr, &err)) return fail(rc, named(i, err));
    }
    HIPCHK(hipSetDevice(ctxs[0]->device));
    // What a context holds of an earlier setup goes: borrows dropped, an arena of its own freed; a layout context gives its 8-byte
    // trip records back, which no kernel of its reads (a set's items have none; a later 1D setup runs on step records).
    auto let_go = [&]() {
        // (nothing of an earlier run in flight on what goes or is written over; a single context waits as it always did: where it
        // gives trip records back, and else in the hipFree of what it owns)
        const hipError_t e = single && !(dims[0] != 0 && ctxs[0]->d_trip_rec) ? hipSuccess : hipDeviceSynchronize();
        for (uint64_t i = 0; i < n; ++i) {
            gfs::free_sgd_state(ctxs[i]);
            if (dims[i] != 0) { ctxs[i]->d_trip_rec.reset(); ctxs[i]->record_facts.have_trip_rec = false; }
        }
        return e;
    };
    // A single context is let go BEFORE it is planned: the plan reads have_trip_rec, and a refusal leaves the context not set up.
    if (single) HIPCHK(let_go());

    // 1. host: every item's launch shape, kernels and schedule; then where its state arrays lie
    std::vector<gfs::SetupPlan> plans(n);
    int refused = GFS_OK;                                                  // a single context's: returned once its replica is there; its plan is one of nothing to do
    for (uint64_t i = 0; i < n; ++i) {
        const int rc = gfs::plan_setup(ctxs[i], params[i], dims[i], cfgs ? &cfgs[i] : nullptr, etas, &plans[i], &err);
        if (rc < 0 && !single) return fail(rc, item_prefix(i) + err);
        if (rc < 0) refused = rc;
    }
    if (single && plans[0].x_len) {                                        // its zeroed replica, whatever the policy said: a refused shape keeps it.
        gfs_ctx *c = ctxs[0];                                              // Before the tables: the memset runs under the host's zeta sum
        hipError_t e = c->d_x.grow(plans[0].x_len * 8);
        if (e == hipSuccess) e = hipMemset(c->d_x, 0, plans[0].x_len * 8);
        if (e != hipSuccess) { gfs::commit_setup(c, std::move(plans[0])); return fail(GFS_E_HIP, std::string("positions: ") + hipGetErrorString(e)); }   // (the plan committed, as it always was)
    }
    constexpr int K = gfs::SET_STATE_KINDS;
    std::vector<uint64_t> bytes(K * n), offsets(K * n);
    gfs_ctx_set_setup_info info{};
    info.items = n;
    std::vector<gfs::SeedItem> seeds;                                      // the items with streams (rng: filled in once the arena is there)
    std::vector<uint64_t> seed_of;                                         // ... and which items they are
    uint64_t total_blocks = 0, most_blocks = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const gfs::SetupPlan &sp = plans[i];
        for (int k = 0; k < K; ++k) bytes[K * i + k] = gfs::state_bytes(sp, (uint32_t)k);
        if (single) bytes[K * i + GFS_STATE_POSITIONS] = 0;                // (an allocation of its own, above)
        if (sp.rc != GFS_OK) { ++info.nothing_to_do; continue; }
        ++info.configured;
        info.total_streams += sp.shape.n_streams;
        const uint64_t nb = (sp.shape.n_streams + gfs::SEED_BLOCK - 1) / gfs::SEED_BLOCK;
        seeds.push_back(gfs::SeedItem{nullptr, sp.params.seed + sp.cfg.stream_base, (uint32_t)sp.shape.n_streams, (uint32_t)total_blocks});
        seed_of.push_back(i);
        total_blocks += nb;
        most_blocks = std::max(most_blocks, nb);
        if (total_blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "set items 0.." + std::to_string(i) + " have more streams together than one seeding launch holds");
    }
    // the arena: [positions, counters, team state, traces, trace counts | RNG words | zeta tables, schedule tables, seeding tables
    // (set_seed_tables.h)]
    const uint64_t arrays_end = gfs::set_state_plan(bytes.data(), n, offsets.data());
    const uint64_t zero_end = gfs::set_state_kind_begin(offsets.data(), GFS_STATE_RNG);
    const uint64_t upload_begin = gfs::set_state_kind_begin(offsets.data(), GFS_STATE_ZETAS);
    const gfs::SeedTables tables = gfs::seed_tables_plan(arrays_end, seeds.size(), sizeof(gfs::SeedItem), total_blocks, most_blocks);
    const uint64_t arena_bytes = tables.end, stage_bytes = arena_bytes - upload_begin;
    info.state_bytes = arena_bytes;

    // ---- from here on a set's items are touched: a failure leaves every context not set up and the arena released ----
    if (!single) HIPCHK(let_go());                                         // (a set only AFTER every item is planned: a refusal above left all as they were)
    int rc = GFS_OK;
    auto ok = [&rc, &arena](const std::string &what, hipError_t e) {       // false: rc holds the reported error, the arena is gone
        if (e == hipSuccess) return true;
        (void)hipDeviceSynchronize();
        arena.reset();
        rc = fail(GFS_E_HIP, what + ": " + hipGetErrorString(e));
        return false;
    };
    if (arena.bytes < arena_bytes) {
        ++info.device_allocations;
        if ((rc = arena.reserve(arena_bytes, ("hipMalloc " + set + "state arena").c_str()))) return rc;
    }
    std::vector<unsigned char> pageable(single ? stage_bytes : 0);         // a single context's staging: no hipHostMalloc per setup
    if (!single && pinned->bytes < stage_bytes) {
        ++info.device_allocations;
        if ((rc = pinned->reserve(stage_bytes, "hipHostMalloc set state staging"))) { arena.reset(); return rc; }
    }
    unsigned char *d_arena = arena.as<unsigned char>(), *h = single ? pageable.data() : pinned->as<unsigned char>();
    auto staged = [h, upload_begin](uint64_t arena_offset) { return h + (arena_offset - upload_begin); };

    // 2. zeta tables: items that share (theta, space_max, step) get slices of one running sum — or the caller's table as it is;
    // 3. staging: the tables, the schedule tables and the seeding kernel's tables, where the arena has them
    if (stage_bytes && !single) std::memset(h, 0, stage_bytes);            // (the zero padding of every zeta table up to zlen_full; pageable: zeroed when made)
    {
        std::vector<gfs_sgd_params> clamped(n);
        std::vector<uint8_t> has_work(n, 0), summed(n, 0);
        for (uint64_t i = 0; i < n; ++i) {
            if (plans[i].rc != GFS_OK) continue;
            clamped[i] = plans[i].params;
            clamped[i].space = gfs::zeta_clamped_space(plans[i].params, plans[i].shape.zlen_staged);
            has_work[i] = 1; summed[i] = zetas == nullptr;
        }
        const gfs::SharedZetaTables shared = gfs::shared_zeta_tables(clamped.data(), summed.data(), n);
        for (uint64_t i = 0; i < n; ++i) {
            if (!has_work[i]) continue;
            const gfs::SetupPlan &sp = plans[i];
            double *table = reinterpret_cast<double *>(staged(offsets[K * i + GFS_STATE_ZETAS]));
            if (zetas) std::memcpy(table, zetas, sp.shape.zlen_full * sizeof(double));
            else gfs::zeta_slice(shared.tables[shared.table_of[i]], clamped[i], sp.shape.zlen_full, table);
            if (bytes[K * i + GFS_STATE_SCHEDULE])
                gfs::schedule_table(sp.params, sp.etas, sp.shape, reinterpret_cast<gfs::IterConsts *>(staged(offsets[K * i + GFS_STATE_SCHEDULE])));
        }
    }
    for (size_t k = 0; k < seeds.size(); ++k) seeds[k].rng = reinterpret_cast<uint64_t *>(d_arena + offsets[K * seed_of[k] + GFS_STATE_RNG]);
    if (!seeds.empty()) gfs::fill_seed_tables(tables, seeds.data(), seeds.size(), gfs::SEED_BLOCK, staged(tables.items_at));

    // 4. one memset over everything a setup zeroes; one copy (blocking from pageable staging); 5. one launch over the concatenated streams
    if (zero_end) {
        if (!ok("hipMemset " + set + "state", hipMemsetAsync(d_arena, 0, zero_end, 0))) return rc;
        ++info.launches;
    }
    if (stage_bytes) {
        if (!ok("hipMemcpy " + set + "state", single ? hipMemcpy(d_arena + upload_begin, h, stage_bytes, hipMemcpyHostToDevice)
                                                     : hipMemcpyAsync(d_arena + upload_begin, h, stage_bytes, hipMemcpyHostToDevice, 0))) return rc;
        ++info.copies;
    }
    if (total_blocks) {
        if (!ok("set_seed_streams_kernel", gfs::seed_streams_device(reinterpret_cast<const gfs::SeedItem *>(d_arena + tables.items_at),
                                                                    reinterpret_cast<const uint32_t *>(d_arena + tables.blocks_at), (uint32_t)total_blocks, 0))) return rc;
        ++info.launches;
    }
    if (!ok("hipDeviceSynchronize", hipDeviceSynchronize())) return rc;     // (the staging is free again; a fault shows here)

    for (uint64_t i = 0, k = 0; i < n; ++i) {
        gfs_ctx *c = ctxs[i];
        const uint64_t *at = &offsets[K * i], *size = &bytes[K * i];
        auto lend = [d_arena, at, size](gfs::Buffer &b, uint32_t kind) { if (size[kind]) (void)b.borrow(d_arena + at[kind]); };
        const bool has_work = plans[i].rc == GFS_OK;
        if (item_rc) item_rc[i] = plans[i].rc;
        gfs::commit_setup(c, std::move(plans[i]));
        lend(c->d_x, GFS_STATE_POSITIONS); lend(c->d_counters, GFS_STATE_COUNTERS); lend(c->d_lead, GFS_STATE_LEAD);
        lend(c->d_trace, GFS_STATE_TRACE); lend(c->d_trace_cnt, GFS_STATE_TRACE_COUNTS); lend(c->d_rng, GFS_STATE_RNG);
        lend(c->d_zetas, GFS_STATE_ZETAS); lend(c->d_its_all, GFS_STATE_SCHEDULE);
        if (has_work) {
            (void)c->d_seed_item.borrow(d_arena + tables.alone_at + k++ * sizeof(gfs::SeedItem));
            (void)c->d_seed_blocks.borrow(d_arena + tables.zeros_at);
        }
        c->configured = refused == GFS_OK;
    }
    if (refused) return fail(refused, err);
    info.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info_out) *info_out = info;
    return GFS_OK;
}

static int set_setup(gfs_ctx_set *s, const std::vector<const gfs_sgd_params *> &params, const std::vector<int> &dims,
                     const gfs_launch_config *cfgs, int32_t *item_rc) {
    std::vector<gfs_ctx *> ctxs;
    for (auto &c : s->items) ctxs.push_back(c.get());
    return gfs::setup_contexts(ctxs.data(), params.data(), dims.data(), cfgs, ctxs.size(), s->state_arena, &s->h_stage, nullptr, nullptr, item_rc,
                               &s->setup_info);
}

extern "C" {

int gfs_ctx_set_state_plan(const uint64_t *bytes, uint64_t n, uint64_t *offsets, uint64_t *arena_bytes) {
    if (!arena_bytes || (n && (!bytes || !offsets))) return fail(GFS_E_ARG, "null argument");
    *arena_bytes = gfs::set_state_plan(bytes, n, offsets);
    return GFS_OK;
}

int gfs_ctx_set_setup_1d(gfs_ctx_set *s, const gfs_sgd_params *params, const gfs_launch_config *cfgs, int32_t *item_rc) {
    if (!s) return fail(GFS_E_ARG, "set is null");
    if (!params) return fail(GFS_E_ARG, "params is null");
    const uint64_t n = s->items.size();
    std::vector<const gfs_sgd_params *> p(n);
    for (uint64_t i = 0; i < n; ++i) p[i] = &params[i];
    return set_setup(s, p, std::vector<int>(n, 0), cfgs, item_rc);
}
int gfs_ctx_set_setup_nd(gfs_ctx_set *s, const gfs_layout_params *params, const gfs_launch_config *cfgs, int32_t *item_rc) {
    if (!s) return fail(GFS_E_ARG, "set is null");
    if (!params) return fail(GFS_E_ARG, "params is null");
    const uint64_t n = s->items.size();
    std::vector<const gfs_sgd_params *> p(n);
    std::vector<int> dims(n);
    for (uint64_t i = 0; i < n; ++i) {
        p[i] = &params[i].sgd;
        dims[i] = params[i].dimensions >= 1 && params[i].dimensions <= GFS_MAX_DIMS ? (int)params[i].dimensions : -1;   // (-1: refused by set_setup, in item order)
    }
    return set_setup(s, p, dims, cfgs, item_rc);
}
int gfs_ctx_set_get_setup_info(const gfs_ctx_set *s, gfs_ctx_set_setup_info *out) {
    if (!s || !out) return fail(GFS_E_ARG, "null argument");
    *out = s->setup_info;
    return GFS_OK;
}

int gfs_ctx_set_plan(const uint64_t *n_nodes, const uint64_t *n_steps, const uint64_t *n_paths, uint64_t n, uint64_t *offsets,
                     uint64_t *arena_bytes) {
    if (!n_nodes || !n_steps || !n_paths || !offsets || !arena_bytes) return fail(GFS_E_ARG, "null argument");
    *arena_bytes = gfs::set_arena_plan(n_nodes, n_steps, n_paths, n, offsets);
    return GFS_OK;
}

void gfs_ctx_set_destroy(gfs_ctx_set *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;                                       // (the items, what their setups allocated, then the arena: the device is set)
}

uint64_t gfs_ctx_set_size(const gfs_ctx_set *s) { return s ? s->items.size() : 0; }
gfs_ctx *gfs_ctx_set_item(gfs_ctx_set *s, uint64_t i) { return s && i < s->items.size() ? s->items[i].get() : nullptr; }
int gfs_ctx_set_get_info(const gfs_ctx_set *s, gfs_ctx_set_info *out) {
    if (!s || !out) return fail(GFS_E_ARG, "null argument");
    *out = s->info;
    return GFS_OK;
}

int gfs_ctx_set_create(const gfs_graph_view *const *graphs, uint64_t n, int device, gfs_ctx_set **out) {
    if (!out) return fail(GFS_E_ARG, "out is null");
    *out = nullptr;
    if (!graphs || n == 0) return fail(GFS_E_ARG, "a context set needs at least one graph view");
    const auto t0 = std::chrono::steady_clock::now();
    // counts first (no array is read), the sums with them; then the arrays.  Each pass names its lowest failing item.
    uint64_t N = 0, S = 0, P = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!graphs[i]) return fail(GFS_E_ARG, item_prefix(i) + "null graph view");
        if (int rc = gfs::check_view_counts(graphs[i], item_prefix(i))) return rc;
        N += graphs[i]->n_nodes; S += graphs[i]->n_steps; P += graphs[i]->n_paths;
        if (N > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "set items 0.." + std::to_string(i) + " have more than 2^31-1 nodes together");
        if (P > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "set items 0.." + std::to_string(i) + " have more than 2^31-1 paths together");
        if (S > (1ull << 40)) return fail(GFS_E_UNSUPPORTED, "set items 0.." + std::to_string(i) + " have more than 2^40 path steps together");
    }
    if (n > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "more than 2^31-1 items");
    for (uint64_t i = 0; i < n; ++i)
        if (int rc = gfs::check_view_paths(graphs[i], item_prefix(i))) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GFS_E_HIP, "no HIP device available (libgfasort_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GFS_E_ARG, "bad device index");
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(GFS_E_HIP, "hipGetDeviceProperties failed");

    // (every error return below relies on scope: the set goes with its items and its arena)
    std::unique_ptr<gfs_ctx_set, decltype(&gfs_ctx_set_destroy)> owner(new (std::nothrow) gfs_ctx_set(), gfs_ctx_set_destroy);
    gfs_ctx_set *s = owner.get();
    if (!s) return fail(GFS_E_NOMEM, "out of memory");
    s->device = device;
    s->items.reserve(n);
    std::vector<gfs_ctx *> ctxs(n);
    for (uint64_t i = 0; i < n; ++i) {
        s->items.emplace_back(new (std::nothrow) gfs_ctx());
        gfs_ctx *c = ctxs[i] = s->items.back().get();
        if (!c) return fail(GFS_E_NOMEM, "out of memory");
        c->device = device; c->cu_count = prop.multiProcessorCount;
        c->set_item = true;
        c->n_nodes = graphs[i]->n_nodes; c->n_steps = graphs[i]->n_steps; c->n_paths = graphs[i]->n_paths;
        if (int rc = gfs::path_facts(graphs[i], c, item_prefix(i))) return rc;
    }
    if (int rc = gfs::build_contexts(graphs, ctxs.data(), n, s->arena, nullptr, true, nullptr, &s->info)) return rc;
    s->info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = owner.release();
    return GFS_OK;
}

}  // extern "C"
