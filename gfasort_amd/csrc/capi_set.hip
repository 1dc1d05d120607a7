// capi_set.hip — the context sets of the C ABI (include/gfasort_hip.h, gfs_ctx_set_*): many gfs_ctx (capi.hip, capi_ctx.h) built
// from many graph views in ONE pass over their disjoint union (K3b, index_set_kernels.hip), and the driver of that build, which
// gfs_ctx_create shares: a single context is a set of one.  The items' index arrays live in one arena the set owns, the items
// borrow them; what a setup allocates stays each item's own.
#include "capi_ctx.h"
#include "index_set.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>

struct gfs_ctx_set {
    int device = 0;
    gfs::Buffer arena;                              // every item's step records, path records, path lengths, node layout, node lengths
    std::vector<std::unique_ptr<gfs_ctx>> items;    // (declared after the arena: they go first)
    gfs_ctx_set_info info{};
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
    uint32_t bad_item = gfs::SET_NO_BAD_ITEM;
    e = gfs::index_set_layout_device(u, d_in + in.bytes, node_perm != nullptr, &bad_item, &info->launches);
    lap("node layout");
    if (e == hipSuccess && bad_item == gfs::SET_NO_BAD_ITEM) e = gfs::index_set_records_device(u, d_in + in.bytes, &info->launches);
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

extern "C" {

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
