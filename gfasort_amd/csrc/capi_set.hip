// capi_set.hip — the context sets of the C ABI (include/gfasort_hip.h, gfs_ctx_set_*): many gfs_ctx (capi.hip, capi_ctx.h) built
// from many graph views in ONE pass over their disjoint union (K3b, index_set_kernels.hip).  The items' index arrays live in one
// arena the set owns, the items borrow them; what a setup allocates stays each item's own.
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
constexpr uint64_t round256(uint64_t b) { return (b + 255ull) & ~255ull; }
constexpr int KINDS = 5;                           // step_rec, path_rec, path_len, perm, node_len
uint64_t kind_bytes(int kind, uint64_t N, uint64_t S, uint64_t P) {
    switch (kind) {
    case 0: return (S + 1) * sizeof(uint4);         // (one record of padding, as gfs_ctx_create allocates)
    case 1: return std::max<uint64_t>(P, 1) * sizeof(uint4);
    case 2: return std::max<uint64_t>(P, 1) * 8;
    case 3: return std::max<uint64_t>(N, 1) * 4;
    default: return std::max<uint64_t>(N, 1) * 4;
    }
}
std::string item_prefix(uint64_t i) { return "set item " + std::to_string(i) + ": "; }
}  // namespace

extern "C" {

int gfs_ctx_set_plan(const uint64_t *n_nodes, const uint64_t *n_steps, const uint64_t *n_paths, uint64_t n, uint64_t *offsets,
                     uint64_t *arena_bytes) {
    if (!n_nodes || !n_steps || !n_paths || !offsets || !arena_bytes) return fail(GFS_E_ARG, "null argument");
    // by kind, then by item: the node lengths of all items (and their layouts) are one range of the arena, one copy each
    uint64_t at = 0;
    for (int kind = 0; kind < KINDS; ++kind)
        for (uint64_t i = 0; i < n; ++i) {
            offsets[KINDS * i + kind] = at;
            at += round256(kind_bytes(kind, n_nodes[i], n_steps[i], n_paths[i]));
        }
    *arena_bytes = at;
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

    // (every error return below relies on scope: the temporaries go first, then the set with its items and its arena)
    std::unique_ptr<gfs_ctx_set, decltype(&gfs_ctx_set_destroy)> owner(new (std::nothrow) gfs_ctx_set(), gfs_ctx_set_destroy);
    gfs_ctx_set *s = owner.get();
    if (!s) return fail(GFS_E_NOMEM, "out of memory");
    s->device = device;
    s->items.reserve(n);
    std::vector<uint64_t> counts(3 * n), offsets(KINDS * n);
    for (uint64_t i = 0; i < n; ++i) {
        s->items.emplace_back(new (std::nothrow) gfs_ctx());
        gfs_ctx *c = s->items.back().get();
        if (!c) return fail(GFS_E_NOMEM, "out of memory");
        c->device = device; c->cu_count = prop.multiProcessorCount;
        c->set_item = true;
        c->n_nodes = graphs[i]->n_nodes; c->n_steps = graphs[i]->n_steps; c->n_paths = graphs[i]->n_paths;
        if (int rc = gfs::path_facts(graphs[i], c, item_prefix(i))) return rc;
        counts[i] = c->n_nodes; counts[n + i] = c->n_steps; counts[2 * n + i] = c->n_paths;
    }
    uint64_t arena_bytes = 0;
    if (int rc = gfs_ctx_set_plan(counts.data(), counts.data() + n, counts.data() + 2 * n, n, offsets.data(), &arena_bytes)) return rc;
    const uint64_t perm_begin = offsets[3], nlen_begin = offsets[4];      // (by kind: the layouts end where the node lengths begin)
    const uint64_t perm_bytes = nlen_begin - perm_begin, nlen_bytes = arena_bytes - nlen_begin;

    // staging, and its mirror at the head of the device scratch: [step_node | path_first | item table | step_is_rev], one copy up;
    // the node lengths go from the staging's tail straight to their range of the arena; the layouts come back into the staging
    const uint64_t at_first = round256(S * 4), at_items = at_first + round256((P + 1) * 8);
    const uint64_t at_rev = at_items + round256((n + 1) * sizeof(gfs::SetItem)), in_bytes = at_rev + round256(S);
    uint64_t work_bytes = 0;
    hipError_t e = gfs::index_set_work_bytes(N, S, &work_bytes);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("rocPRIM temporary storage: ") + hipGetErrorString(e));
    gfs::Buffer h_stage{true}, d_scratch;                                  // (freed after the synchronise that ends the build)
    int rc = GFS_OK;
    if ((rc = s->arena.reserve(std::max<uint64_t>(arena_bytes, 256), "hipMalloc set arena"))) return rc;
    if ((rc = d_scratch.reserve(in_bytes + work_bytes, "hipMalloc set scratch"))) return rc;
    if ((rc = h_stage.reserve(std::max(in_bytes + nlen_bytes, perm_bytes), "hipHostMalloc set staging"))) return rc;
    s->info.device_allocations = 3;
    auto ok = [&rc](const char *what, hipError_t err) {                    // false: rc holds the reported error
        if (err != hipSuccess) rc = fail(GFS_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
        return err == hipSuccess;
    };
    if (!ok("hipMemset set arena", hipMemsetAsync(s->arena.p, 0, std::max<uint64_t>(arena_bytes, 256), 0))) return rc;
    ++s->info.launches;

    unsigned char *h = h_stage.as<unsigned char>();
    auto *h_step_node = reinterpret_cast<uint32_t *>(h);
    auto *h_first = reinterpret_cast<uint64_t *>(h + at_first);
    auto *h_items = reinterpret_cast<gfs::SetItem *>(h + at_items);
    uint8_t *h_rev = h + at_rev;
    unsigned char *h_nlen = h + in_bytes;
    std::memset(h_nlen, 0, nlen_bytes);
    uint64_t node_off = 0, step_off = 0, path_off = 0;
    for (uint64_t i = 0; i <= n; ++i) {
        gfs::SetItem &it = h_items[i];
        it = gfs::SetItem{node_off, step_off, path_off, 0, 0, 0, 0, 0};
        if (i == n) break;
        const gfs_graph_view *g = graphs[i];
        it.rec = offsets[KINDS * i]; it.prec = offsets[KINDS * i + 1]; it.plen = offsets[KINDS * i + 2];
        it.perm = offsets[KINDS * i + 3]; it.nlen = offsets[KINDS * i + 4];
        if (g->n_steps) {
            std::memcpy(h_step_node + step_off, g->step_node, g->n_steps * 4);
            std::memcpy(h_rev + step_off, g->step_is_rev, g->n_steps);
        }
        for (uint64_t p = 0; p < g->n_paths; ++p) h_first[path_off + p] = step_off + g->path_first_step[p];
        if (g->n_nodes) std::memcpy(h_nlen + (it.nlen - nlen_begin), g->node_len, g->n_nodes * 4);
        node_off += g->n_nodes; step_off += g->n_steps; path_off += g->n_paths;
    }
    h_first[P] = S;
    unsigned char *d_in = d_scratch.as<unsigned char>(), *d_arena = s->arena.as<unsigned char>();
    if (!ok("hipMemcpy set inputs", hipMemcpyAsync(d_in, h, in_bytes, hipMemcpyHostToDevice, 0))) return rc;
    if (nlen_bytes && !ok("hipMemcpy set node_len", hipMemcpyAsync(d_arena + nlen_begin, h_nlen, nlen_bytes, hipMemcpyHostToDevice, 0))) return rc;

    gfs::SetUnion u{};
    u.n_items = (uint32_t)n; u.n_nodes = N; u.n_steps = S; u.n_paths = P;
    u.step_node = reinterpret_cast<const uint32_t *>(d_in);
    u.path_first = reinterpret_cast<const uint64_t *>(d_in + at_first);
    u.items = reinterpret_cast<const gfs::SetItem *>(d_in + at_items);
    u.step_is_rev = d_in + at_rev;
    u.arena = d_arena;
    uint32_t bad_item = gfs::SET_NO_BAD_ITEM;
    e = gfs::build_index_set_device(u, d_in + in_bytes, &bad_item, &s->info.launches);
    if (e != hipSuccess || bad_item != gfs::SET_NO_BAD_ITEM) (void)hipDeviceSynchronize();   // (nothing in flight when the buffers go)
    if (!ok("build_index_set", e)) return rc;
    if (bad_item != gfs::SET_NO_BAD_ITEM) return fail(GFS_E_ARG, item_prefix(bad_item) + "step_node out of range");
    // every item's layout back in one copy (blocking: it ends the build)
    if (!ok("hipMemcpy set perm", hipMemcpy(h, d_arena + perm_begin, std::max<uint64_t>(perm_bytes, 4), hipMemcpyDeviceToHost))) return rc;
    if (!ok("hipDeviceSynchronize", hipDeviceSynchronize())) return rc;
    for (uint64_t i = 0; i < n; ++i) {
        gfs_ctx *c = s->items[i].get();
        const uint32_t *perm = reinterpret_cast<const uint32_t *>(h + (offsets[KINDS * i + 3] - perm_begin));
        c->perm.assign(perm, perm + c->n_nodes);
        (void)c->d_step_rec.borrow(d_arena + offsets[KINDS * i]);
        (void)c->d_path_rec.borrow(d_arena + offsets[KINDS * i + 1]);
        (void)c->d_path_len.borrow(d_arena + offsets[KINDS * i + 2]);
        (void)c->d_perm.borrow(d_arena + offsets[KINDS * i + 3]);
        (void)c->d_node_len.borrow(d_arena + offsets[KINDS * i + 4]);
    }
    s->info.items = n; s->info.total_nodes = N; s->info.total_steps = S; s->info.total_paths = P;
    s->info.arena_bytes = arena_bytes;
    s->info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = owner.release();
    return GFS_OK;
}

}  // extern "C"
