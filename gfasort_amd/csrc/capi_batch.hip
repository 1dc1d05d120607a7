// capi_batch.hip — the batch entries of the C ABI (include/gfasort_hip.h, gfs_batch_*): many configured contexts (capi.hip,
// capi_ctx.h) in one persistent launch (K1f / K2f, sgd_kernels_batch.hip), and their start positions, read-outs, coordinates and
// pair errors in one launch each (K4b / K6b, K4c / K6c, K7g), and their diagnosis — errors per path, stretched pairs, errors per node —
// and their sort quality in a constant number of launches (K7h, K7i, K7j; K7k).
#include "capi_ctx.h"
#include "sgd_batch.h"
#include "batch_plan.h"
#include "batch_readout_plan.h"
#include "segment_sort.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <numeric>

struct BatchLaunch {
    bool lds_tables = false;
    size_t lds_bytes = 0;              // the largest among its items
    uint64_t first = 0, count = 0;     // its items: run[first .. first + count)
    uint64_t blocks = 0, block_offset = 0;   // workgroups; where its part of the block table starts
    gfs::EventPair ev;                 // created with the batch
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
    gfs::Buffer d_items, d_block_item, d_pool;       // BatchItem table, block table, every item's pool counters: sized at create
    uint64_t launches_done = 0, blocks_done = 0;
    double kernel_ms = 0.0, total_ms = 0.0;
    // K4b / K6b (batch_readout_kernels.hip): the item table, the packed outputs and the per-item sort's scratch, allocated on first use
    uint64_t sort_cap = gfs::SEGMENT_SORT_CAP;       // items of more nodes take K6, one by one (gfs_batch_debug_sort_cap)
    std::vector<gfs::ReadoutItem> h_readout;
    gfs::Buffer d_readout, d_positions, d_order, d_sort_tmp;
    gfs::Buffer h_packed{true};        // pinned staging of every read-out: copies land here at full rate, whatever the caller's pages are
    gfs::EventPair readout_timer;      // created on first use: start and stop on the stream, read after the synchronise
    // K4c / K6c and K7g (batch_quality_kernels.hip): one device buffer each, [what the host sends | what the kernels write], grown on demand
    gfs::Buffer d_coords, d_quality;   // (d_quality is also K7h-j's, batch_diagnosis_kernels.hip: tables, scratch, the scan's storage, results)
    uint64_t tile_blocks = 0;          // gfs_batch_debug_tile_blocks: a cap on K7h's and K7i's grids, 0 = none
};
static_assert(GFS_SEGMENT_SORT_CAP == gfs::SEGMENT_SORT_CAP, "the header's cap is the network's");

static void read_kernel_ms(const gfs::EventPair &timer, double *kernel_ms) {
    float t = 0.f;
    if (kernel_ms && timer.elapsed(&t)) *kernel_ms = t;
}
static bool batch_item_idle(const gfs_ctx *c) { return !c->valid_paths || c->n_nodes == 0; }
static bool batch_eligible(const gfs_ctx *c) {
    return gfs::batch_eligible(c->shape, c->cfg.trace_per_stream != 0, c->d_its_all != nullptr, batch_item_idle(c));
}

extern "C" {

void gfs_batch_destroy(gfs_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;                                                              // (its buffers and events go here: the device is set)
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
        int rc = b->d_items.reserve(b->run.size() * sizeof(gfs::BatchItem), "hipMalloc items");
        if (!rc) rc = b->d_block_item.reserve(b->total_blocks * sizeof(uint32_t), "hipMalloc block table");
        if (!rc) rc = b->d_pool.reserve(b->pool_words * sizeof(uint32_t), "hipMalloc pools");
        if (rc) { gfs_batch_destroy(b); return rc; }
        for (auto &l : b->launches)
            if ((rc = l.ev.ready())) { gfs_batch_destroy(b); return rc; }
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
            it.a.it = gfs::iter_consts(c, 0);
            it.its = c->d_its_all;
            it.pool = b->d_pool.as<uint32_t>() + b->pool_offset[r];
            it.n_iters = (uint32_t)(c->params.iter_max + 1);
            it.first_block = (uint32_t)block;
            const uint64_t nb = b->item_blocks[r];
            for (uint64_t k = 0; k < nb; ++k) b->h_block_item[l.block_offset + block + k] = (uint32_t)r;
            block += nb;
        }
    }
    HIPCHK(hipMemcpyAsync(b->d_items.p, b->h_items.data(), b->h_items.size() * sizeof(gfs::BatchItem), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_block_item.p, b->h_block_item.data(), b->h_block_item.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // work pools (sgd_kernel_common.h pool_walk): every item's counters, zeroed per run
    HIPCHK(hipMemsetAsync(b->d_pool.p, 0, b->pool_words * sizeof(uint32_t), st));
    for (BatchLaunch &l : b->launches) {
        const gfs::BatchItem *items = b->d_items.as<gfs::BatchItem>();
        const uint32_t *block_item = b->d_block_item.as<uint32_t>() + l.block_offset;
        void *args[] = {&items, &block_item};
        HIPCHK(l.ev.start(st));                          // (the event pair brackets the kernel alone)
        hipError_t e = hipLaunchKernel(gfs::batch_fused_kernel(b->dims, l.lds_tables), dim3((unsigned)l.blocks), dim3(b->block), args, l.lds_bytes, st);
        if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch kernel launch: ") + hipGetErrorString(e));
        HIPCHK(l.ev.stop(st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (BatchLaunch &l : b->launches) {
        float t = 0.f;
        if (l.ev.elapsed(&t)) b->kernel_ms += t;
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
// where each item starts in the packed outputs (the nodes of the items before it); one entry more than items: the total
static std::vector<uint64_t> batch_offsets(const gfs_batch *b) {
    std::vector<uint64_t> offsets(b->ctxs.size() + 1, 0);
    for (size_t i = 0; i < b->ctxs.size(); ++i) offsets[i + 1] = offsets[i] + b->ctxs[i]->n_nodes;
    return offsets;
}
static std::vector<uint64_t> batch_nodes(const gfs_batch *b) {
    std::vector<uint64_t> nodes(b->ctxs.size());
    for (size_t i = 0; i < nodes.size(); ++i) nodes[i] = b->ctxs[i]->n_nodes;
    return nodes;
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
    if (int rc = b->d_readout.reserve(b->ctxs.size() * sizeof(gfs::ReadoutItem))) return rc;
    const std::vector<uint64_t> offset = batch_offsets(b);
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
        HIPCHK(hipMemcpyAsync(b->d_readout.p, b->h_readout.data(), order.size() * sizeof(gfs::ReadoutItem), hipMemcpyHostToDevice, st));
    return GFS_OK;
}

int gfs_batch_result_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n) {
    if (!b || !offsets) return fail(GFS_E_ARG, "null argument");
    if (n != b->ctxs.size() + 1) return fail(GFS_E_ARG, "offsets: need items + 1 entries");
    const std::vector<uint64_t> of = batch_offsets(b);
    std::copy(of.begin(), of.end(), offsets);
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
    hipError_t e = gfs::batch_init_positions_device(b->d_readout.as<gfs::ReadoutItem>(), (uint32_t)all.size(), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch init_positions: ") + hipGetErrorString(e));
    HIPCHK(hipStreamSynchronize(st));
    return GFS_OK;
}

int gfs_batch_results(gfs_batch *b, double *positions, uint32_t *order, uint64_t total, double *kernel_ms, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    if (!positions && !order) return fail(GFS_E_ARG, "both output buffers are null");
    if (total != batch_offsets(b).back()) return fail(GFS_E_ARG, "total is not the batch's node count (gfs_batch_result_offsets)");
    int rc = batch_readout_check(b);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_sort_order
    hipStream_t st = (hipStream_t)hip_stream;
    rc = b->d_positions.reserve(total * sizeof(double));
    if (!rc) rc = b->d_order.reserve(total * sizeof(uint32_t));
    if (rc) return rc;
    double *const d_positions = b->d_positions.as<double>();
    uint32_t *const d_order = b->d_order.as<uint32_t>();
    // items within the cap by the length of their padded segment: one launch per length, its LDS and block sized by it; the others after them
    const std::vector<uint64_t> nodes = batch_nodes(b);
    std::vector<uint64_t> by_len(nodes.size());
    const uint64_t within = gfs::segment_launch_order(nodes.data(), nodes.size(), b->sort_cap, by_len.data());
    rc = batch_readout_table(b, by_len, st);
    if (rc) return rc;
    HIPCHK(b->readout_timer.start(st));
    for (uint64_t first = 0; first < within;) {
        const uint64_t P = gfs::segment_group_of(nodes[by_len[first]], b->sort_cap);
        const uint64_t end = gfs::segment_launch_end(nodes.data(), by_len.data(), first, within, b->sort_cap);
        for (uint64_t at = first; at < end; at += 0x7FFFFFFFull) {         // (a grid's x dimension)
            const uint32_t count = (uint32_t)std::min<uint64_t>(end - at, 0x7FFFFFFFull);
            hipError_t e = gfs::sort_segments_device(b->d_readout.as<gfs::ReadoutItem>() + at, count, (uint32_t)P, positions ? d_positions : nullptr, d_order, st);
            if (e != hipSuccess) return fail(GFS_E_HIP, std::string("segment sort launch: ") + hipGetErrorString(e));
        }
        first = end;
    }
    // above the cap: K6 (rocPRIM radix sort) once each, into the same packed arrays
    for (size_t r = within; r < by_len.size(); ++r) {
        const gfs_ctx *c = b->ctxs[by_len[r]];
        const gfs::ReadoutItem &it = b->h_readout[r];
        const uint64_t n = c->n_nodes, need = n * (2 * 8 + 2 * 4);
        HIPCHK(hipStreamSynchronize(st));                                  // (K6 runs on the null stream)
        rc = b->d_sort_tmp.reserve(need);
        if (rc) return rc;
        uint32_t *d_sorted = nullptr;
        hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, n, 1, b->d_sort_tmp.p, &d_sorted);
        if (e != hipSuccess) return fail(GFS_E_HIP, "batch item " + std::to_string(by_len[r]) + ": sort_order_device: " + hipGetErrorString(e));
        HIPCHK(hipMemcpyAsync(d_order + it.offset, d_sorted, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (positions) {
            e = gfs::reorder_positions_device(c->d_x, d_positions + it.offset, c->d_perm, n, 0, 0, st);
            if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch positions: ") + hipGetErrorString(e));
        }
        HIPCHK(hipStreamSynchronize(st));                                  // (the scratch is the next item's)
    }
    HIPCHK(b->readout_timer.stop(st));
    // The two copies go through pinned memory of the batch: a copy of megabytes straight into the caller's pageable buffer has
    // the runtime pin those pages first, 20-30 ms where they are fresh (profiles/r10/batch_readout_probe_pageable.log).
    rc = b->h_packed.reserve(total * (sizeof(double) + sizeof(uint32_t)));
    if (rc) return rc;
    double *h_positions = b->h_packed.as<double>();
    uint32_t *h_order = reinterpret_cast<uint32_t *>(h_positions + total);
    if (positions && total) HIPCHK(hipMemcpyAsync(h_positions, d_positions, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (order && total) HIPCHK(hipMemcpyAsync(h_order, d_order, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (positions && total) std::memcpy(positions, h_positions, total * sizeof(double));
    if (order && total) std::memcpy(order, h_order, total * sizeof(uint32_t));
    read_kernel_ms(b->readout_timer, kernel_ms);
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
    int rc = b->h_packed.reserve(bytes);
    if (!rc) rc = b->d_coords.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_coords.as<unsigned char>();
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
    HIPCHK(b->readout_timer.start(st));
    hipError_t e = gfs::batch_coords_device(reinterpret_cast<const gfs::CoordItem *>(d + tables_at), reinterpret_cast<const uint32_t *>(d + blocks_at),
                                            blocks, reinterpret_cast<double *>(d), to_device, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch coordinates launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    if (!to_device) HIPCHK(hipMemcpyAsync(h, d, total * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!to_device) std::memcpy(coords, h, total * sizeof(double));
    read_kernel_ms(b->readout_timer, kernel_ms);
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
    int rc = gfs::check_step_distances(zs, n_z, out);
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
    rc = b->h_packed.reserve(out_at + out_bytes);                          // (staging: the same offsets, less the partials)
    if (!rc) rc = b->d_quality.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_quality.as<unsigned char>();
    std::memcpy(h, zs, n_z * 8);
    gfs::QualityItem *h_items = reinterpret_cast<gfs::QualityItem *>(h + items_at);
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::QualityItem{c->d_step_rec, c->d_x, c->n_steps, c->n_nodes, (uint32_t)first_block[i], (uint32_t)(first_block[i + 1] - first_block[i])};
    }
    gfs::block_item_table(first_block.data(), n, reinterpret_cast<uint32_t *>(h + blocks_at));
    HIPCHK(hipMemcpyAsync(d, h, blocks_at + row_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(b->readout_timer.start(st));
    hipError_t e = gfs::batch_pair_errors_device(reinterpret_cast<const gfs::QualityItem *>(d + items_at), reinterpret_cast<const uint32_t *>(d + blocks_at),
                                                 (uint32_t)n, row_blocks, (uint32_t)b->dims, reinterpret_cast<const uint64_t *>(d), (uint32_t)n_z,
                                                 reinterpret_cast<uint64_t *>(d + partials_at), reinterpret_cast<uint64_t *>(d + out_at), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch pair_errors launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    HIPCHK(hipMemcpyAsync(h + out_at, d + out_at, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t *w = reinterpret_cast<const uint64_t *>(h + out_at);
    for (uint64_t r = 0; r < n * n_z; ++r) out[r] = gfs::unpack_pair_error(zs[r % n_z], &w[5 * r]);
    read_kernel_ms(b->readout_timer, kernel_ms);
    return GFS_OK;
}

// ---- K7k: gfs_ctx_sort_quality of every item of a batch of 1D sorts (batch_sort_quality_kernels.hip) ------------------------------
static uint64_t words8(uint64_t bytes) { return (bytes + 7) / 8 * 8; }

int gfs_batch_sort_quality(gfs_batch *b, gfs_sort_quality *out, uint64_t n, double *kernel_ms, void *hip_stream) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    if (!out) return fail(GFS_E_ARG, "out is null");
    if (n != b->ctxs.size()) return fail(GFS_E_ARG, "n is not the batch's item count");
    if (b->dims != 0) return fail(GFS_E_UNSUPPORTED, "a batch of layouts has no sort quality (dims=" + std::to_string(b->dims) +
                                                          "): use gfs_batch_pair_errors and gfs_batch_path_errors");
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        if (c->dims != 0 || (c->n_nodes && !c->d_x)) return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": needs a 1D context that has been set up");
    }
    if (n > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's items exceed one table");
    const std::vector<uint64_t> nodes = batch_nodes(b), first_node = batch_offsets(b);
    std::vector<uint64_t> steps(n), first_block(n + 1), by_len(n);
    for (uint64_t i = 0; i < n; ++i) steps[i] = b->ctxs[i]->n_steps;
    const uint64_t row_blocks = gfs::quality_plan(steps.data(), n, first_block.data()), total_nodes = first_node.back();
    if (row_blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's step tables exceed one launch");
    const uint64_t within = gfs::segment_launch_order(nodes.data(), n, b->sort_cap, by_len.data());
    if (kernel_ms) *kernel_ms = 0.0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_sort_quality: nothing of an item is in flight
    hipStream_t st = (hipStream_t)hip_stream;
    // device: [ReadoutItem rows, in launch order | SortQualityItem table | block table (whole words) | out words | totals by row |
    // sorted positions, packed by item | partials]; the first three go up in one copy, out and totals come back in one
    const uint64_t items_at = n * sizeof(gfs::ReadoutItem), blocks_at = items_at + n * sizeof(gfs::SortQualityItem);
    const uint64_t out_at = blocks_at + words8(row_blocks * sizeof(uint32_t)), totals_at = out_at + n * 5 * 8, spos_at = totals_at + n * 8;
    const uint64_t partials_at = spos_at + total_nodes * 8, bytes = partials_at + 5 * row_blocks * 8;
    int rc = b->h_packed.reserve(spos_at);                                 // (staging: the same offsets, less positions and partials)
    if (!rc) rc = b->d_quality.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_quality.as<unsigned char>();
    uint64_t *const d_spos = reinterpret_cast<uint64_t *>(d + spos_at), *const d_totals = reinterpret_cast<uint64_t *>(d + totals_at);
    gfs::ReadoutItem *h_rows = reinterpret_cast<gfs::ReadoutItem *>(h);
    gfs::SortQualityItem *h_items = reinterpret_cast<gfs::SortQualityItem *>(h + items_at);
    for (uint64_t r = 0; r < n; ++r) {                                     // from the contexts as they are now (positions may have been bound anew)
        const gfs_ctx *c = b->ctxs[by_len[r]];
        gfs::ReadoutItem &it = h_rows[r];
        it.x = c->d_x; it.perm = c->d_perm; it.node_len = c->d_node_len;
        it.offset = first_node[by_len[r]];
        it.n = (uint32_t)c->n_nodes;                                       // (a context has fewer than 2^31 nodes)
        it.padded = r < within ? (uint32_t)gfs::segment_group_of(c->n_nodes, b->sort_cap) : 0;
    }
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::SortQualityItem{c->d_step_rec, d_spos + first_node[i], c->n_steps, (uint32_t)first_block[i], (uint32_t)(first_block[i + 1] - first_block[i])};
    }
    gfs::block_item_table(first_block.data(), n, reinterpret_cast<uint32_t *>(h + blocks_at));
    HIPCHK(hipMemcpyAsync(d, h, blocks_at + row_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(b->readout_timer.start(st));
    for (uint64_t first = 0; first < within;) {
        const uint64_t P = gfs::segment_group_of(nodes[by_len[first]], b->sort_cap);
        const uint64_t end = gfs::segment_launch_end(nodes.data(), by_len.data(), first, within, b->sort_cap);
        hipError_t e = gfs::batch_sorted_positions_device(reinterpret_cast<const gfs::ReadoutItem *>(d) + first, (uint32_t)(end - first), (uint32_t)P, d_spos,
                                                          d_totals + first, st);
        if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch sorted positions launch: ") + hipGetErrorString(e));
        first = end;
    }
    // above the cap: K6 and K7c's own scan and scatter once each, into the same packed positions
    std::vector<uint64_t> long_total(n - within, 0);
    for (uint64_t r = within; r < n; ++r) {
        const gfs_ctx *c = b->ctxs[by_len[r]];
        const uint64_t nn = c->n_nodes, sort_bytes = nn * (2 * 8 + 2 * 4);
        HIPCHK(hipStreamSynchronize(st));                                  // (K6 runs on the null stream)
        rc = b->d_sort_tmp.reserve(sort_bytes + (nn + 1) * 8);             // [K6's scratch | prefix]
        if (rc) return rc;
        uint32_t *d_sorted = nullptr;
        hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, nn, 1, b->d_sort_tmp.p, &d_sorted);
        if (e != hipSuccess) return fail(GFS_E_HIP, "batch item " + std::to_string(by_len[r]) + ": sort_order_device: " + hipGetErrorString(e));
        e = gfs::sorted_positions_device(d_sorted, c->d_node_len, c->d_perm, nn, reinterpret_cast<uint64_t *>(b->d_sort_tmp.as<unsigned char>() + sort_bytes),
                                         d_spos + first_node[by_len[r]], &long_total[r - within], st);
        if (e != hipSuccess) return fail(GFS_E_HIP, "batch item " + std::to_string(by_len[r]) + ": sorted_positions_device: " + hipGetErrorString(e));
        HIPCHK(hipStreamSynchronize(st));                                  // (the scratch is the next item's)
    }
    hipError_t e = gfs::batch_sort_quality_device(reinterpret_cast<const gfs::SortQualityItem *>(d + items_at), reinterpret_cast<const uint32_t *>(d + blocks_at),
                                                  (uint32_t)n, row_blocks, reinterpret_cast<uint64_t *>(d + partials_at), reinterpret_cast<uint64_t *>(d + out_at), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch sort_quality launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    HIPCHK(hipMemcpyAsync(h + out_at, d + out_at, spos_at - out_at, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    read_kernel_ms(b->readout_timer, kernel_ms);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(h + out_at), *totals = reinterpret_cast<const uint64_t *>(h + totals_at);
    for (uint64_t r = 0; r < n; ++r)
        if ((r < within ? totals[r] : long_total[r - within]) >= (1ull << 53))
            return fail(GFS_E_UNSUPPORTED, "batch item " + std::to_string(by_len[r]) + ": a graph of 2^53 bp or more");
    for (uint64_t i = 0; i < n; ++i) {
        out[i].steps = w[5 * i]; out[i].abs_err_sum = w[5 * i + 1]; out[i].genomic_sum = w[5 * i + 2];
        std::memcpy(&out[i].sq_err_sum, &w[5 * i + 3], 8);
    }
    return GFS_OK;
}

// ---- K7h / K7i / K7j: gfs_ctx_path_errors, gfs_ctx_stretched_pairs and gfs_ctx_node_errors of every item ---------------------------
// Where every item's tiles, paths, nodes, listed pairs and step-pass workgroups start (batch_readout_plan.h), from the contexts as
// they are now.
struct DiagPlan {
    std::vector<uint64_t> steps, first_tile, first_path, first_node, first_pair, first_block;
    uint64_t tiles = 0, paths = 0, nodes = 0, pairs = 0, row_blocks = 0;
};
static DiagPlan diag_plan(const gfs_batch *b, uint64_t cap) {
    const uint64_t n = b->ctxs.size();
    DiagPlan p;
    std::vector<uint64_t> paths(n), nodes(n);
    p.steps.resize(n);
    for (uint64_t i = 0; i < n; ++i) { p.steps[i] = b->ctxs[i]->n_steps; paths[i] = b->ctxs[i]->n_paths; nodes[i] = b->ctxs[i]->n_nodes; }
    for (std::vector<uint64_t> *v : {&p.first_tile, &p.first_path, &p.first_node, &p.first_pair, &p.first_block}) v->resize(n + 1);
    p.tiles = gfs::tile_plan(p.steps.data(), n, p.first_tile.data());
    p.paths = gfs::row_offsets(paths.data(), n, p.first_path.data());
    p.nodes = gfs::row_offsets(nodes.data(), n, p.first_node.data());
    p.pairs = gfs::stretched_list_plan(p.steps.data(), n, cap, p.first_pair.data());
    p.row_blocks = gfs::quality_plan(p.steps.data(), n, p.first_block.data());
    return p;
}
static void diag_items(const gfs_batch *b, const DiagPlan &p, gfs::DiagItem *items) {
    for (uint64_t i = 0; i < b->ctxs.size(); ++i) {
        const gfs_ctx *c = b->ctxs[i];
        items[i] = gfs::DiagItem{c->d_step_rec, c->d_path_rec, c->d_x, c->d_perm, c->n_steps, c->n_nodes, c->n_paths, p.first_tile[i], p.first_path[i],
                                 p.first_node[i], p.first_pair[i], (uint32_t)p.first_block[i], (uint32_t)(p.first_block[i + 1] - p.first_block[i])};
    }
}
// gfs_ctx_*'s rules for z and ratio, then every item's state; no device call
static int diag_check(const gfs_batch *b, uint64_t z, double ratio) {
    int rc = gfs::check_diagnosis(z, ratio);
    if (rc) return rc;
    for (size_t i = 0; i < b->ctxs.size(); ++i)
        if (!b->ctxs[i]->d_x || b->ctxs[i]->dims != b->dims)
            return fail(GFS_E_STATE, "batch item " + std::to_string(i) + ": the context has no positions (not set up) or is no longer of the batch's dimensions");
    if (b->ctxs.size() > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's items exceed one table");
    return GFS_OK;
}

int gfs_batch_path_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n) {
    if (!b || !offsets) return fail(GFS_E_ARG, "null argument");
    if (n != b->ctxs.size() + 1) return fail(GFS_E_ARG, "offsets: need items + 1 entries");
    offsets[0] = 0;
    for (size_t i = 0; i < b->ctxs.size(); ++i) offsets[i + 1] = offsets[i] + b->ctxs[i]->n_paths;
    return GFS_OK;
}

int gfs_batch_debug_tile_blocks(gfs_batch *b, uint64_t max_blocks) {
    if (!b) return fail(GFS_E_ARG, "batch is null");
    b->tile_blocks = max_blocks;
    return GFS_OK;
}

int gfs_batch_path_errors(gfs_batch *b, uint64_t z, double ratio, gfs_path_error *out, uint64_t total_paths, double *kernel_ms, void *hip_stream) {
    if (!b || (!out && total_paths)) return fail(GFS_E_ARG, "null argument");
    int rc = diag_check(b, z, ratio);
    if (rc) return rc;
    const DiagPlan p = diag_plan(b, 0);
    if (total_paths != p.paths) return fail(GFS_E_ARG, "total_paths is not the batch's path count (gfs_batch_path_offsets)");
    if (kernel_ms) *kernel_ms = 0.0;
    if (p.paths == 0) return GFS_OK;
    static_assert(sizeof(gfs_path_error) == 8 * 8, "K7h writes gfs_path_error as 8 words");
    const uint64_t n = b->ctxs.size();
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // device: [DiagItem table | tile table (whole words) | out | head partials | tail partials]; the first two go up in one copy
    const uint64_t tiles_at = n * sizeof(gfs::DiagItem), out_at = tiles_at + words8(p.tiles * sizeof(uint32_t)), out_bytes = p.paths * sizeof(gfs_path_error);
    const uint64_t head_at = out_at + out_bytes, tail_at = head_at + 5 * p.tiles * 8, bytes = tail_at + 5 * p.tiles * 8;
    rc = b->h_packed.reserve(out_at + out_bytes);                          // (staging: the same offsets, less the partials)
    if (!rc) rc = b->d_quality.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_quality.as<unsigned char>();
    diag_items(b, p, reinterpret_cast<gfs::DiagItem *>(h));
    gfs::tile_item_table(p.first_tile.data(), n, reinterpret_cast<uint32_t *>(h + tiles_at));
    HIPCHK(hipMemcpyAsync(d, h, out_at, hipMemcpyHostToDevice, st));
    HIPCHK(b->readout_timer.start(st));
    hipError_t e = gfs::batch_path_errors_device(reinterpret_cast<const gfs::DiagItem *>(d), reinterpret_cast<const uint32_t *>(d + tiles_at), (uint32_t)n,
                                                 p.tiles, p.paths, (uint32_t)b->dims, z, ratio, reinterpret_cast<uint64_t *>(d + head_at),
                                                 reinterpret_cast<uint64_t *>(d + tail_at), reinterpret_cast<uint64_t *>(d + out_at), b->tile_blocks, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch path_errors launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    HIPCHK(hipMemcpyAsync(h + out_at, d + out_at, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(out, h + out_at, out_bytes);
    read_kernel_ms(b->readout_timer, kernel_ms);
    return GFS_OK;
}

int gfs_batch_stretched_pairs(gfs_batch *b, uint64_t z, double ratio, gfs_stretched_pair *out, uint64_t cap, uint64_t *totals, double *kernel_ms,
                              void *hip_stream) {
    if (!b || !totals || (!out && cap)) return fail(GFS_E_ARG, "null argument");
    int rc = diag_check(b, z, ratio);
    if (rc) return rc;
    const uint64_t n = b->ctxs.size();
    for (uint64_t i = 0; i < n; ++i) totals[i] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const DiagPlan p = diag_plan(b, cap);
    if (p.tiles == 0) return GFS_OK;
    static_assert(sizeof(gfs_stretched_pair) == 5 * 8, "K7i writes gfs_stretched_pair as 5 words");
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    size_t tmp_bytes = 0;
    hipError_t e = gfs::batch_stretched_scan_bytes(p.tiles, &tmp_bytes);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch stretched_pairs scan: ") + hipGetErrorString(e));
    // device: [DiagItem table | tile table (whole words) | tile counts | offsets | list | the scan's storage]; the first two go up in one
    // copy, offsets and list come back in one
    const uint64_t tiles_at = n * sizeof(gfs::DiagItem), counts_at = tiles_at + words8(p.tiles * sizeof(uint32_t));
    const uint64_t offsets_at = counts_at + (p.tiles + 1) * 8, list_at = offsets_at + (p.tiles + 1) * 8;
    const uint64_t tmp_at = list_at + p.pairs * sizeof(gfs_stretched_pair), bytes = tmp_at + (tmp_bytes ? tmp_bytes : 8);
    rc = b->h_packed.reserve(tmp_at);                                      // (staging: the same offsets, less the scan's storage)
    if (!rc) rc = b->d_quality.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_quality.as<unsigned char>();
    diag_items(b, p, reinterpret_cast<gfs::DiagItem *>(h));
    gfs::tile_item_table(p.first_tile.data(), n, reinterpret_cast<uint32_t *>(h + tiles_at));
    HIPCHK(hipMemcpyAsync(d, h, counts_at, hipMemcpyHostToDevice, st));
    HIPCHK(b->readout_timer.start(st));
    e = gfs::batch_stretched_pairs_device(reinterpret_cast<const gfs::DiagItem *>(d), reinterpret_cast<const uint32_t *>(d + tiles_at), p.tiles,
                                          (uint32_t)b->dims, z, ratio, reinterpret_cast<uint64_t *>(d + counts_at), reinterpret_cast<uint64_t *>(d + offsets_at),
                                          p.pairs ? d + list_at : nullptr, cap, d + tmp_at, tmp_bytes, b->tile_blocks, st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch stretched_pairs launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    HIPCHK(hipMemcpyAsync(h + offsets_at, d + offsets_at, tmp_at - offsets_at, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t *offsets = reinterpret_cast<const uint64_t *>(h + offsets_at);
    const gfs_stretched_pair *list = reinterpret_cast<const gfs_stretched_pair *>(h + list_at);
    for (uint64_t i = 0; i < n; ++i) {
        totals[i] = offsets[p.first_tile[i + 1]] - offsets[p.first_tile[i]];
        const uint64_t listed = std::min(std::min(cap, p.steps[i]), totals[i]);
        if (listed) std::memcpy(out + i * cap, list + p.first_pair[i], listed * sizeof(gfs_stretched_pair));
    }
    read_kernel_ms(b->readout_timer, kernel_ms);
    return GFS_OK;
}

int gfs_batch_node_errors(gfs_batch *b, uint64_t z, double ratio, gfs_node_error *out, uint64_t total_nodes, double *kernel_ms, void *hip_stream) {
    if (!b || (!out && total_nodes)) return fail(GFS_E_ARG, "null argument");
    int rc = diag_check(b, z, ratio);
    if (rc) return rc;
    const DiagPlan p = diag_plan(b, 0);
    if (total_nodes != p.nodes) return fail(GFS_E_ARG, "total_nodes is not the batch's node count (gfs_batch_result_offsets)");
    if (p.row_blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's step tables exceed one launch");
    if (kernel_ms) *kernel_ms = 0.0;
    if (p.nodes == 0) return GFS_OK;
    static_assert(sizeof(gfs_node_error) == 3 * 8, "K7j writes gfs_node_error as 3 words");
    const uint64_t n = b->ctxs.size();
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // device: [DiagItem table | block table (whole words) | out | per slot: pairs, stretched, max]; the first two go up in one copy
    const uint64_t blocks_at = n * sizeof(gfs::DiagItem), out_at = blocks_at + words8(p.row_blocks * sizeof(uint32_t));
    const uint64_t out_bytes = p.nodes * sizeof(gfs_node_error), slots_at = out_at + out_bytes, bytes = slots_at + out_bytes;
    rc = b->h_packed.reserve(out_at + out_bytes);                          // (staging: the same offsets, less the slots)
    if (!rc) rc = b->d_quality.reserve(bytes);
    if (rc) return rc;
    unsigned char *h = b->h_packed.as<unsigned char>(), *d = b->d_quality.as<unsigned char>();
    diag_items(b, p, reinterpret_cast<gfs::DiagItem *>(h));
    gfs::block_item_table(p.first_block.data(), n, reinterpret_cast<uint32_t *>(h + blocks_at));
    HIPCHK(hipMemcpyAsync(d, h, out_at, hipMemcpyHostToDevice, st));
    HIPCHK(b->readout_timer.start(st));
    hipError_t e = gfs::batch_node_errors_device(reinterpret_cast<const gfs::DiagItem *>(d), reinterpret_cast<const uint32_t *>(d + blocks_at), (uint32_t)n,
                                                 p.row_blocks, p.nodes, (uint32_t)b->dims, z, ratio, reinterpret_cast<uint64_t *>(d + slots_at),
                                                 reinterpret_cast<uint64_t *>(d + out_at), st);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch node_errors launch: ") + hipGetErrorString(e));
    HIPCHK(b->readout_timer.stop(st));
    HIPCHK(hipMemcpyAsync(h + out_at, d + out_at, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(out, h + out_at, out_bytes);
    read_kernel_ms(b->readout_timer, kernel_ms);
    return GFS_OK;
}

}  // extern "C"
