// capi_batch.hip — the batch entries of the C ABI (include/gfasort_hip.h, gfs_batch_*): many configured contexts (capi.hip,
// capi_ctx.h) in one persistent launch (K1f / K2f, sgd_kernels_batch.hip), and their start positions, read-outs, coordinates and
// pair errors in one launch each (K4b / K6b, K4c / K6c, K7g), and their diagnosis — errors per path, stretched pairs, errors per node —
// and their sort quality in a constant number of launches (K7h, K7i, K7j; K7k).
// A read-out maps its one allocation with a gfs::Region (readout_region.h) and makes one RoundTrip through it; its checks, its plan,
// its table fill, its launch and its unpacking are its own.
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

static bool batch_item_idle(const gfs_ctx *c) { return !c->valid_paths || c->n_nodes == 0; }
static bool batch_eligible(const gfs_ctx *c) {
    return gfs::batch_eligible(c->shape, c->cfg.trace_per_stream != 0, c->d_its_all != nullptr, batch_item_idle(c));
}

// one count of every item (&gfs_ctx::n_nodes, n_steps, n_paths), as the plans of batch_readout_plan.h take them
static std::vector<uint64_t> item_counts(const gfs_batch *b, uint64_t gfs_ctx::*count) {
    std::vector<uint64_t> counts(b->ctxs.size());
    for (size_t i = 0; i < counts.size(); ++i) counts[i] = b->ctxs[i]->*count;
    return counts;
}
// where each item's rows start in an output packed by node (or by path); one entry more than items: the total
static std::vector<uint64_t> batch_offsets(const gfs_batch *b, uint64_t gfs_ctx::*count = &gfs_ctx::n_nodes) {
    const std::vector<uint64_t> counts = item_counts(b, count);
    std::vector<uint64_t> offsets(counts.size() + 1);
    gfs::row_offsets(counts.data(), counts.size(), offsets.data());
    return offsets;
}
// the row of K4b / K6b / K7k for context c as it is now (positions may have been bound anew; it has fewer than 2^31 nodes)
static gfs::ReadoutItem readout_row(const gfs_ctx *c, uint64_t offset, uint32_t padded) { return {c->d_x, c->d_perm, c->d_node_len, offset, (uint32_t)c->n_nodes, padded}; }

// One read-out's round trip through one allocation mapped by a gfs::Region (readout_region.h): a device buffer of the batch and, for
// the parts up to staged(), the batch's pinned staging at the same offsets.  An entry reserves, fills the tables in h, uploads them
// (the timer starts), launches, and finishes: the launch's verdict, the timer's stop, the results back into h, the wait, kernel_ms.
struct GFS_LOCAL RoundTrip {
    gfs_batch *b; hipStream_t st;
    unsigned char *h = nullptr, *d = nullptr;                              // the staging and the device buffer, once reserved
    template <typename T> T *host(uint64_t part) const { return gfs::Region::at<T>(h, part); }
    template <typename T> T *device(uint64_t part) const { return gfs::Region::at<T>(d, part); }
    int reserve(const gfs::Region &map, gfs::Buffer *dev) {                // (dev null: the staging alone)
        int rc = b->h_packed.reserve(map.staged());
        if (!rc && dev) rc = dev->reserve(map.bytes());
        h = b->h_packed.as<unsigned char>(); d = dev ? dev->as<unsigned char>() : nullptr;
        return rc;
    }
    int start() { HIPCHK(b->readout_timer.start(st)); return GFS_OK; }
    int upload(uint64_t from, uint64_t to) {                               // ... and the timer's start behind it
        HIPCHK(hipMemcpyAsync(d + from, h + from, to - from, hipMemcpyHostToDevice, st));
        return start();
    }
    int finish(hipError_t launched, const char *what, uint64_t from, uint64_t to, double *kernel_ms) {
        if (launched != hipSuccess) return fail(GFS_E_HIP, std::string(what) + ": " + hipGetErrorString(launched));
        HIPCHK(b->readout_timer.stop(st));
        if (to > from) HIPCHK(hipMemcpyAsync(h + from, d + from, to - from, hipMemcpyDeviceToHost, st));
        return wait(kernel_ms);
    }
    int wait(double *kernel_ms) {
        HIPCHK(hipStreamSynchronize(st));
        float t = 0.f;
        if (kernel_ms && b->readout_timer.elapsed(&t)) *kernel_ms = t;
        return GFS_OK;
    }
};

// One launch per padded segment length (K6b, K7k): launch(first, end, padded) for the rows [first, end) of by_len, which share it.
template <typename Launch>
static int for_each_segment_launch(const std::vector<uint64_t> &nodes, const std::vector<uint64_t> &by_len, uint64_t within, uint64_t cap, Launch launch) {
    for (uint64_t first = 0, end; first < within; first = end) {
        end = gfs::segment_launch_end(nodes.data(), by_len.data(), first, within, cap);
        if (int rc = launch(first, end, (uint32_t)gfs::segment_group_of(nodes[by_len[first]], cap))) return rc;
    }
    return GFS_OK;
}
// An item above the sort cap: K6 (rocPRIM radix sort) for it alone, in the batch's sort scratch with `extra` bytes of the caller's behind
// K6's own, then then(c, d_sorted, those bytes) on st.  Two waits: K6 runs on the null stream, and the scratch is the next item's.
template <typename Then>
static int sort_item_above_cap(gfs_batch *b, uint64_t item, uint64_t extra, hipStream_t st, Then then) {
    const gfs_ctx *c = b->ctxs[item];
    const uint64_t sort_bytes = gfs::sort_order_scratch_bytes(c->n_nodes);
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = b->d_sort_tmp.reserve(sort_bytes + extra)) return rc;
    uint32_t *d_sorted = nullptr;
    hipError_t e = gfs::sort_order_device(c->d_x, c->d_perm, c->n_nodes, 1, b->d_sort_tmp.p, &d_sorted);
    if (e != hipSuccess) return fail(GFS_E_HIP, "batch item " + std::to_string(item) + ": sort_order_device: " + hipGetErrorString(e));
    if (int rc = then(c, d_sorted, b->d_sort_tmp.as<unsigned char>() + sort_bytes)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return GFS_OK;
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
// The item table from the contexts as they are now, in the order `order` lists them; offsets are those of gfs_batch_result_offsets.
// Uploaded on st.
static int batch_readout_table(gfs_batch *b, const std::vector<uint64_t> &order, hipStream_t st) {
    if (int rc = b->d_readout.reserve(b->ctxs.size() * sizeof(gfs::ReadoutItem))) return rc;
    const std::vector<uint64_t> offset = batch_offsets(b);
    b->h_readout.resize(order.size());
    for (size_t r = 0; r < order.size(); ++r) {
        const gfs_ctx *c = b->ctxs[order[r]];
        b->h_readout[r] = readout_row(c, offset[order[r]], c->n_nodes <= gfs::SEGMENT_SORT_CAP ? gfs::segment_padded((uint32_t)c->n_nodes) : 0);
    }
    if (!order.empty())
        HIPCHK(hipMemcpyAsync(b->d_readout.p, b->h_readout.data(), order.size() * sizeof(gfs::ReadoutItem), hipMemcpyHostToDevice, st));
    return GFS_OK;
}
static int copy_offsets(const std::vector<uint64_t> &of, uint64_t *offsets, uint64_t n) {
    if (n != of.size()) return fail(GFS_E_ARG, "offsets: need items + 1 entries");
    std::copy(of.begin(), of.end(), offsets);
    return GFS_OK;
}

int gfs_batch_result_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n) {
    if (!b || !offsets) return fail(GFS_E_ARG, "null argument");
    return copy_offsets(batch_offsets(b), offsets, n);
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
    if ((rc = batch_readout_table(b, all, st))) return rc;
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
    const std::vector<uint64_t> nodes = item_counts(b, &gfs_ctx::n_nodes);
    std::vector<uint64_t> by_len(nodes.size());
    const uint64_t within = gfs::segment_launch_order(nodes.data(), nodes.size(), b->sort_cap, by_len.data());
    if ((rc = batch_readout_table(b, by_len, st))) return rc;
    RoundTrip rt{b, st};
    if ((rc = rt.start())) return rc;
    rc = for_each_segment_launch(nodes, by_len, within, b->sort_cap, [&](uint64_t first, uint64_t end, uint32_t padded) -> int {
        for (uint64_t at = first; at < end; at += 0x7FFFFFFFull) {         // (a grid's x dimension)
            const uint32_t count = (uint32_t)std::min<uint64_t>(end - at, 0x7FFFFFFFull);
            hipError_t e = gfs::sort_segments_device(b->d_readout.as<gfs::ReadoutItem>() + at, count, padded, positions ? d_positions : nullptr, d_order, st);
            if (e != hipSuccess) return fail(GFS_E_HIP, std::string("segment sort launch: ") + hipGetErrorString(e));
        }
        return GFS_OK;
    });
    // above the cap: K6 once each, into the same packed arrays
    for (size_t r = within; r < by_len.size() && !rc; ++r)
        rc = sort_item_above_cap(b, by_len[r], 0, st, [&](const gfs_ctx *c, const uint32_t *d_sorted, void *) -> int {
            const uint64_t offset = b->h_readout[r].offset;
            HIPCHK(hipMemcpyAsync(d_order + offset, d_sorted, c->n_nodes * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
            if (!positions) return GFS_OK;
            hipError_t e = gfs::reorder_positions_device(c->d_x, d_positions + offset, c->d_perm, c->n_nodes, 0, 0, st);
            return e == hipSuccess ? GFS_OK : fail(GFS_E_HIP, std::string("batch positions: ") + hipGetErrorString(e));
        });
    if (rc) return rc;
    HIPCHK(b->readout_timer.stop(st));
    // The two copies go through pinned memory of the batch: a copy of megabytes straight into the caller's pageable buffer has
    // the runtime pin those pages first, 20-30 ms where they are fresh (profiles/r10/batch_readout_probe_pageable.log).
    gfs::Region map;                                                       // the staging alone: [positions | order]
    const uint64_t positions_at = map.add(total * sizeof(double)), order_at = map.add(total * sizeof(uint32_t));   map.end_staging();
    if ((rc = rt.reserve(map, nullptr))) return rc;
    if (positions && total) HIPCHK(hipMemcpyAsync(rt.h + positions_at, d_positions, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (order && total) HIPCHK(hipMemcpyAsync(rt.h + order_at, d_order, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if ((rc = rt.wait(kernel_ms))) return rc;
    if (positions && total) std::memcpy(positions, rt.h + positions_at, total * sizeof(double));
    if (order && total) std::memcpy(order, rt.h + order_at, total * sizeof(uint32_t));
    return GFS_OK;
}

// ---- K4c / K6c: every item's layout coordinates, up or down, in one launch and one copy of coordinates -------------------------
// The checks of both directions, on every item; no device call.
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
// One call either way: up, the whole region goes in one copy; down, the two tables go up and the coordinates come back.
static int batch_coords_move(gfs_batch *b, double *coords, uint64_t total, int to_device, double *kernel_ms, hipStream_t st) {
    int rc = batch_coords_check(b, coords, total);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    const uint64_t n = b->ctxs.size();
    const std::vector<uint64_t> nodes = item_counts(b, &gfs_ctx::n_nodes);
    std::vector<uint64_t> word_offset(n + 1), first_block(n + 1);
    const uint64_t blocks = gfs::coord_plan(nodes.data(), n, (uint32_t)b->dims, word_offset.data(), first_block.data());
    if (blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's coordinates exceed one launch");
    if (total == 0) return GFS_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_download_positions: nothing of an item is in flight
    gfs::Region map;                                                       // [packed coordinates | CoordItem table | block table]
    const uint64_t coords_at = map.add(total * sizeof(double)), items_at = map.add(n * sizeof(gfs::CoordItem));
    const uint64_t blocks_at = map.add(blocks * sizeof(uint32_t));   map.end_upload(); map.end_staging();
    RoundTrip rt{b, st};
    if ((rc = rt.reserve(map, &b->d_coords))) return rc;
    gfs::CoordItem *h_items = rt.host<gfs::CoordItem>(items_at);
    for (uint64_t i = 0; i < n; ++i) {                                     // from the contexts as they are now (positions may have been bound anew)
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::CoordItem{c->d_x, c->d_perm, word_offset[i], (uint32_t)c->n_nodes, (uint32_t)first_block[i], (uint32_t)b->dims, 0u};
    }
    gfs::block_item_table(first_block.data(), n, rt.host<uint32_t>(blocks_at));
    if (to_device) std::memcpy(rt.h + coords_at, coords, total * sizeof(double));
    if ((rc = rt.upload(to_device ? coords_at : items_at, map.uploaded()))) return rc;
    hipError_t e = gfs::batch_coords_device(rt.device<const gfs::CoordItem>(items_at), rt.device<const uint32_t>(blocks_at), blocks,
                                            rt.device<double>(coords_at), to_device, st);
    if ((rc = rt.finish(e, "batch coordinates launch", coords_at, coords_at + (to_device ? 0 : total * sizeof(double)), kernel_ms))) return rc;
    if (!to_device) std::memcpy(coords, rt.h + coords_at, total * sizeof(double));
    return GFS_OK;
}

int gfs_batch_upload_coords(gfs_batch *b, const double *coords, uint64_t total, void *hip_stream) {
    return batch_coords_move(b, const_cast<double *>(coords), total, 1, nullptr, (hipStream_t)hip_stream);
}

int gfs_batch_coords(gfs_batch *b, double *coords, uint64_t total, double *kernel_ms, void *hip_stream) {
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
    const std::vector<uint64_t> steps = item_counts(b, &gfs_ctx::n_steps);
    std::vector<uint64_t> first_block(n + 1);
    const uint64_t row_blocks = gfs::quality_plan(steps.data(), n, first_block.data());
    if (row_blocks > 0x7FFFFFFFull || n > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's step tables exceed one launch");
    HIPCHK(hipSetDevice(b->device));
    gfs::Region map;                                                       // [zs | QualityItem table | block table] [out words] [partials]
    const uint64_t zs_at = map.add(n_z * 8), items_at = map.add(n * sizeof(gfs::QualityItem)), blocks_at = map.add(row_blocks * sizeof(uint32_t));   map.end_upload();
    const uint64_t out_at = map.add(n * n_z * 5 * 8);   map.end_staging();
    const uint64_t partials_at = map.add(5 * n_z * row_blocks * 8);
    RoundTrip rt{b, (hipStream_t)hip_stream};
    if ((rc = rt.reserve(map, &b->d_quality))) return rc;
    std::memcpy(rt.h + zs_at, zs, n_z * 8);
    gfs::QualityItem *h_items = rt.host<gfs::QualityItem>(items_at);
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::QualityItem{c->d_step_rec, c->d_x, c->n_steps, c->n_nodes, (uint32_t)first_block[i], (uint32_t)(first_block[i + 1] - first_block[i])};
    }
    gfs::block_item_table(first_block.data(), n, rt.host<uint32_t>(blocks_at));
    if ((rc = rt.upload(zs_at, map.uploaded()))) return rc;
    hipError_t e = gfs::batch_pair_errors_device(rt.device<const gfs::QualityItem>(items_at), rt.device<const uint32_t>(blocks_at), (uint32_t)n, row_blocks,
                                                 (uint32_t)b->dims, rt.device<const uint64_t>(zs_at), (uint32_t)n_z, rt.device<uint64_t>(partials_at),
                                                 rt.device<uint64_t>(out_at), rt.st);
    if ((rc = rt.finish(e, "batch pair_errors launch", out_at, map.staged(), kernel_ms))) return rc;
    const uint64_t *w = rt.host<const uint64_t>(out_at);
    for (uint64_t r = 0; r < n * n_z; ++r) out[r] = gfs::unpack_pair_error(zs[r % n_z], &w[5 * r]);
    return GFS_OK;
}

// ---- K7k: gfs_ctx_sort_quality of every item of a batch of 1D sorts (batch_sort_quality_kernels.hip) ------------------------------
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
    const std::vector<uint64_t> nodes = item_counts(b, &gfs_ctx::n_nodes), steps = item_counts(b, &gfs_ctx::n_steps), first_node = batch_offsets(b);
    std::vector<uint64_t> first_block(n + 1), by_len(n);
    const uint64_t row_blocks = gfs::quality_plan(steps.data(), n, first_block.data());
    if (row_blocks > 0x7FFFFFFFull) return fail(GFS_E_UNSUPPORTED, "the batch's step tables exceed one launch");
    const uint64_t within = gfs::segment_launch_order(nodes.data(), n, b->sort_cap, by_len.data());
    if (kernel_ms) *kernel_ms = 0.0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());                                        // as gfs_ctx_sort_quality: nothing of an item is in flight
    hipStream_t st = (hipStream_t)hip_stream;
    // [ReadoutItem rows, in launch order | SortQualityItem table | block table] [out words | totals by row] [sorted positions by item | partials]
    gfs::Region map;
    const uint64_t rows_at = map.add(n * sizeof(gfs::ReadoutItem)), items_at = map.add(n * sizeof(gfs::SortQualityItem));
    const uint64_t blocks_at = map.add(row_blocks * sizeof(uint32_t));   map.end_upload();
    const uint64_t out_at = map.add(n * 5 * 8), totals_at = map.add(n * 8);   map.end_staging();
    const uint64_t spos_at = map.add(first_node.back() * 8), partials_at = map.add(5 * row_blocks * 8);
    RoundTrip rt{b, st};
    int rc = rt.reserve(map, &b->d_quality);
    if (rc) return rc;
    uint64_t *const d_spos = rt.device<uint64_t>(spos_at), *const d_totals = rt.device<uint64_t>(totals_at);
    gfs::ReadoutItem *h_rows = rt.host<gfs::ReadoutItem>(rows_at);
    gfs::SortQualityItem *h_items = rt.host<gfs::SortQualityItem>(items_at);
    for (uint64_t r = 0; r < n; ++r)
        h_rows[r] = readout_row(b->ctxs[by_len[r]], first_node[by_len[r]], r < within ? (uint32_t)gfs::segment_group_of(nodes[by_len[r]], b->sort_cap) : 0);
    for (uint64_t i = 0; i < n; ++i) {
        const gfs_ctx *c = b->ctxs[i];
        h_items[i] = gfs::SortQualityItem{c->d_step_rec, d_spos + first_node[i], c->n_steps, (uint32_t)first_block[i], (uint32_t)(first_block[i + 1] - first_block[i])};
    }
    gfs::block_item_table(first_block.data(), n, rt.host<uint32_t>(blocks_at));
    if ((rc = rt.upload(rows_at, map.uploaded()))) return rc;
    rc = for_each_segment_launch(nodes, by_len, within, b->sort_cap, [&](uint64_t first, uint64_t end, uint32_t padded) -> int {
        hipError_t e = gfs::batch_sorted_positions_device(rt.device<const gfs::ReadoutItem>(rows_at) + first, (uint32_t)(end - first), padded, d_spos, d_totals + first, st);
        return e == hipSuccess ? GFS_OK : fail(GFS_E_HIP, std::string("batch sorted positions launch: ") + hipGetErrorString(e));
    });
    // above the cap: K6 and K7c's own scan and scatter once each, into the same packed positions; behind K6's scratch, the prefix
    std::vector<uint64_t> long_total(n - within, 0);
    for (uint64_t r = within; r < n && !rc; ++r)
        rc = sort_item_above_cap(b, by_len[r], (nodes[by_len[r]] + 1) * 8, st, [&](const gfs_ctx *c, const uint32_t *d_sorted, void *d_prefix) -> int {
            hipError_t e = gfs::sorted_positions_device(d_sorted, c->d_node_len, c->d_perm, c->n_nodes, static_cast<uint64_t *>(d_prefix),
                                                        d_spos + first_node[by_len[r]], &long_total[r - within], st);
            return e == hipSuccess ? GFS_OK : fail(GFS_E_HIP, "batch item " + std::to_string(by_len[r]) + ": sorted_positions_device: " + hipGetErrorString(e));
        });
    if (rc) return rc;
    hipError_t e = gfs::batch_sort_quality_device(rt.device<const gfs::SortQualityItem>(items_at), rt.device<const uint32_t>(blocks_at), (uint32_t)n, row_blocks,
                                                  rt.device<uint64_t>(partials_at), rt.device<uint64_t>(out_at), st);
    if ((rc = rt.finish(e, "batch sort_quality launch", out_at, map.staged(), kernel_ms))) return rc;
    const uint64_t *w = rt.host<const uint64_t>(out_at), *totals = rt.host<const uint64_t>(totals_at);
    for (uint64_t r = 0; r < n; ++r)
        if ((rc = gfs::check_sorted_length(r < within ? totals[r] : long_total[r - within], (int64_t)by_len[r]))) return rc;
    for (uint64_t i = 0; i < n; ++i) out[i] = gfs::unpack_sort_quality(&w[5 * i]);
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
    p.steps = item_counts(b, &gfs_ctx::n_steps);
    p.first_path = batch_offsets(b, &gfs_ctx::n_paths); p.first_node = batch_offsets(b);
    for (std::vector<uint64_t> *v : {&p.first_tile, &p.first_pair, &p.first_block}) v->resize(n + 1);
    p.tiles = gfs::tile_plan(p.steps.data(), n, p.first_tile.data());
    p.paths = p.first_path.back(); p.nodes = p.first_node.back();
    p.pairs = gfs::stretched_list_plan(p.steps.data(), n, cap, p.first_pair.data());
    p.row_blocks = gfs::quality_plan(p.steps.data(), n, p.first_block.data());
    return p;
}
// the two tables every diagnosis sends, filled in the staging and uploaded: the items, and (first_tile or first_block) whose a tile or a workgroup is
static int diag_send(RoundTrip &rt, const gfs::Region &map, const DiagPlan &p, const std::vector<uint64_t> &first, uint64_t items_at, uint64_t table_at) {
    gfs::DiagItem *items = rt.host<gfs::DiagItem>(items_at);
    for (uint64_t i = 0; i < rt.b->ctxs.size(); ++i) {
        const gfs_ctx *c = rt.b->ctxs[i];
        items[i] = gfs::DiagItem{c->d_step_rec, c->d_path_rec, c->d_x, c->d_perm, c->n_steps, c->n_nodes, c->n_paths, p.first_tile[i], p.first_path[i],
                                 p.first_node[i], p.first_pair[i], (uint32_t)p.first_block[i], (uint32_t)(p.first_block[i + 1] - p.first_block[i])};
    }
    gfs::block_item_table(first.data(), rt.b->ctxs.size(), rt.host<uint32_t>(table_at));
    return rt.upload(items_at, map.uploaded());
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
    return copy_offsets(batch_offsets(b, &gfs_ctx::n_paths), offsets, n);
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
    const uint64_t n = b->ctxs.size();
    HIPCHK(hipSetDevice(b->device));
    gfs::Region map;                                                       // [DiagItem table | tile table] [out] [head partials | tail partials]
    const uint64_t items_at = map.add(n * sizeof(gfs::DiagItem)), tiles_at = map.add(p.tiles * sizeof(uint32_t));   map.end_upload();
    const uint64_t out_at = map.add(p.paths * sizeof(gfs_path_error));   map.end_staging();
    const uint64_t head_at = map.add(5 * p.tiles * 8), tail_at = map.add(5 * p.tiles * 8);
    RoundTrip rt{b, (hipStream_t)hip_stream};
    if ((rc = rt.reserve(map, &b->d_quality)) || (rc = diag_send(rt, map, p, p.first_tile, items_at, tiles_at))) return rc;
    hipError_t e = gfs::batch_path_errors_device(rt.device<const gfs::DiagItem>(items_at), rt.device<const uint32_t>(tiles_at), (uint32_t)n, p.tiles, p.paths,
                                                 (uint32_t)b->dims, z, ratio, rt.device<uint64_t>(head_at), rt.device<uint64_t>(tail_at),
                                                 rt.device<uint64_t>(out_at), b->tile_blocks, rt.st);
    if ((rc = rt.finish(e, "batch path_errors launch", out_at, map.staged(), kernel_ms))) return rc;
    std::memcpy(out, rt.h + out_at, p.paths * sizeof(gfs_path_error));
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
    HIPCHK(hipSetDevice(b->device));
    size_t tmp_bytes = 0;
    hipError_t e = gfs::batch_stretched_scan_bytes(p.tiles, &tmp_bytes);
    if (e != hipSuccess) return fail(GFS_E_HIP, std::string("batch stretched_pairs scan: ") + hipGetErrorString(e));
    gfs::Region map;   // [DiagItem table | tile table] [tile counts | offsets | list], of which offsets and list come back, [the scan's storage, never empty]
    const uint64_t items_at = map.add(n * sizeof(gfs::DiagItem)), tiles_at = map.add(p.tiles * sizeof(uint32_t));   map.end_upload();
    const uint64_t counts_at = map.add((p.tiles + 1) * 8), offsets_at = map.add((p.tiles + 1) * 8), list_at = map.add(p.pairs * sizeof(gfs_stretched_pair));   map.end_staging();
    const uint64_t tmp_at = map.add(tmp_bytes ? tmp_bytes : 8);
    RoundTrip rt{b, (hipStream_t)hip_stream};
    if ((rc = rt.reserve(map, &b->d_quality)) || (rc = diag_send(rt, map, p, p.first_tile, items_at, tiles_at))) return rc;
    e = gfs::batch_stretched_pairs_device(rt.device<const gfs::DiagItem>(items_at), rt.device<const uint32_t>(tiles_at), p.tiles, (uint32_t)b->dims, z, ratio,
                                          rt.device<uint64_t>(counts_at), rt.device<uint64_t>(offsets_at), p.pairs ? rt.d + list_at : nullptr, cap,
                                          rt.d + tmp_at, tmp_bytes, b->tile_blocks, rt.st);
    if ((rc = rt.finish(e, "batch stretched_pairs launch", offsets_at, map.staged(), kernel_ms))) return rc;
    const uint64_t *offsets = rt.host<const uint64_t>(offsets_at);
    const gfs_stretched_pair *list = rt.host<const gfs_stretched_pair>(list_at);
    for (uint64_t i = 0; i < n; ++i) {
        totals[i] = offsets[p.first_tile[i + 1]] - offsets[p.first_tile[i]];
        const uint64_t listed = std::min(std::min(cap, p.steps[i]), totals[i]);
        if (listed) std::memcpy(out + i * cap, list + p.first_pair[i], listed * sizeof(gfs_stretched_pair));
    }
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
    const uint64_t n = b->ctxs.size();
    HIPCHK(hipSetDevice(b->device));
    gfs::Region map;                                                       // [DiagItem table | block table] [out] [per slot: pairs, stretched, max]
    const uint64_t items_at = map.add(n * sizeof(gfs::DiagItem)), blocks_at = map.add(p.row_blocks * sizeof(uint32_t));   map.end_upload();
    const uint64_t out_at = map.add(p.nodes * sizeof(gfs_node_error));   map.end_staging();
    const uint64_t slots_at = map.add(p.nodes * sizeof(gfs_node_error));
    RoundTrip rt{b, (hipStream_t)hip_stream};
    if ((rc = rt.reserve(map, &b->d_quality)) || (rc = diag_send(rt, map, p, p.first_block, items_at, blocks_at))) return rc;
    hipError_t e = gfs::batch_node_errors_device(rt.device<const gfs::DiagItem>(items_at), rt.device<const uint32_t>(blocks_at), (uint32_t)n, p.row_blocks, p.nodes,
                                                 (uint32_t)b->dims, z, ratio, rt.device<uint64_t>(slots_at), rt.device<uint64_t>(out_at), rt.st);
    if ((rc = rt.finish(e, "batch node_errors launch", out_at, map.staged(), kernel_ms))) return rc;
    std::memcpy(out, rt.h + out_at, p.nodes * sizeof(gfs_node_error));
    return GFS_OK;
}

}  // extern "C"

