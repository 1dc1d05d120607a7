// sgd.cpp — see sgd.hpp.
#include "sgd.hpp"

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <iostream>
#include <memory>
#include <ostream>
#include <stdexcept>

namespace gfasort {

gfs_sgd_params PathSGDParams::to_c() const {
    gfs_sgd_params c;
    std::memset(&c, 0, sizeof c);
    c.iter_max = iter_max; c.iter_with_max_learning_rate = iter_with_max_learning_rate;
    c.min_term_updates = min_term_updates; c.delta = delta; c.eps = eps; c.eta_max = eta_max; c.theta = theta;
    c.space = space; c.space_max = space_max; c.space_quantization_step = space_quantization_step;
    c.cooling_start = cooling_start; c.nthreads = nthreads; c.progress = progress ? 1 : 0; c.seed = seed;
    return c;
}

gfs_layout_params LayoutSGDParams::to_c() const {
    PathSGDParams s;
    s.iter_max = iter_max; s.iter_with_max_learning_rate = iter_with_max_learning_rate;
    s.min_term_updates = min_term_updates; s.delta = delta; s.eps = eps; s.eta_max = eta_max; s.theta = theta;
    s.space = space; s.space_max = space_max; s.space_quantization_step = space_quantization_step;
    s.cooling_start = cooling_start; s.nthreads = nthreads; s.progress = progress; s.seed = seed;
    gfs_layout_params c;
    c.dimensions = dimensions; c.sgd = s.to_c();
    return c;
}

// path statistics used by both from_graph functions (they each build a throw-away PathIndex
// in the reference: ygs.rs:58, sgd.rs:734)
static void path_stats(const BidirectedGraph &g, uint64_t &sum_steps, size_t &max_steps, size_t &max_len) {
    sum_steps = 0; max_steps = 0; max_len = 0;
    for (const auto &p : g.paths) {
        size_t pos = 0;
        for (Handle h : p.steps) {
            size_t id = h.node_id();
            if (id < g.nodes.size() && g.nodes[id].has_value()) pos += g.nodes[id]->sequence.size();
        }
        sum_steps += p.steps.size();
        max_steps = std::max(max_steps, p.steps.size());
        max_len = std::max(max_len, pos);
    }
}

LayoutSGDParams LayoutSGDParams::from_graph(const BidirectedGraph &g, size_t dimensions, size_t nthreads) {
    uint64_t sum; size_t mx, ml;
    path_stats(g, sum, mx, ml);
    LayoutSGDParams p;
    p.dimensions = dimensions; p.iter_max = 30; p.min_term_updates = 10 * sum;     // sgd.rs:749
    p.eta_max = (double)(mx * mx); p.space = mx; p.space_max = 1000; p.space_quantization_step = 100;
    p.nthreads = nthreads;
    return p;
}

YgsParams::YgsParams() {                                             // ygs.rs:23-45
    path_sgd.iter_max = 100; path_sgd.min_term_updates = 0; path_sgd.eta_max = 0.0; path_sgd.space = 0;
    path_sgd.space_max = 100; path_sgd.space_quantization_step = 100;
}

YgsParams YgsParams::from_graph(const BidirectedGraph &g, uint8_t verbose, size_t nthreads) {
    YgsParams y;
    y.verbose = verbose;
    y.path_sgd.nthreads = nthreads;
    y.path_sgd.progress = verbose >= 2;
    uint64_t sum; size_t mx, ml;
    path_stats(g, sum, mx, ml);
    y.path_sgd.min_term_updates = sum;                               // ygs.rs:73
    y.path_sgd.eta_max = (double)(mx * mx);                          // ygs.rs:76
    y.path_sgd.space = ml;                                           // ygs.rs:79
    if (verbose >= 2) {
        std::cerr << "[ygs_sort] Calculated parameters:\n  sum_path_step_count: " << sum
                  << "\n  max_path_step_count: " << mx << "\n  max_path_length: " << ml
                  << "\n  min_term_updates: " << y.path_sgd.min_term_updates
                  << "\n  eta_max: " << rust_display_f64(y.path_sgd.eta_max) << "\n  space: " << y.path_sgd.space << "\n";
    }
    return y;
}

// ---- Layout ---------------------------------------------------------------------------------------
Layout Layout::from_vectors(const std::vector<std::vector<double>> &v) {
    if (v.empty()) throw std::runtime_error("Must have at least 1 dimension");
    size_t entries = v[0].size();
    if (entries % 2) throw std::runtime_error("Must have even number of entries (2 per node)");
    for (const auto &d : v) if (d.size() != entries) throw std::runtime_error("All dimension vectors must have same length");
    Layout l(v.size(), entries / 2);
    for (size_t node = 0; node < l.num_nodes; ++node)
        for (size_t end = 0; end < 2; ++end)
            for (size_t dim = 0; dim < l.dimensions; ++dim) l.coords[l.index(node, end, dim)] = v[dim][node * 2 + end];
    return l;
}

double Layout::distance(size_t na, size_t ea, size_t nb, size_t eb) const {
    double s = 0.0;
    for (size_t d = 0; d < dimensions; ++d) { double delta = get(na, ea, d) - get(nb, eb, d); s += delta * delta; }
    return std::sqrt(s);
}

std::string rust_display_f64(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[512];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);     // shortest round-trip, no exponent
    return std::string(buf, r.ptr);
}

static const char *dim_name(size_t d) {                              // layout.rs:248-256
    switch (d) { case 0: return "x"; case 1: return "y"; case 2: return "z"; case 3: return "w"; default: return "d"; }
}

void Layout::write_tsv(std::ostream &out) const {
    out << "idx";
    for (size_t d = 0; d < dimensions; ++d) out << "\t" << dim_name(d) << "+";
    for (size_t d = 0; d < dimensions; ++d) out << "\t" << dim_name(d) << "-";
    out << "\n";
    // rows formatted in blocks by the host threads, a window of blocks at a time, written in order
    const size_t BLOCK = 1 << 14, nblocks = (num_nodes + BLOCK - 1) / BLOCK;
    const size_t window = std::max<size_t>(io_threads() * 4, 1);
    std::vector<std::string> piece(std::min(window, std::max<size_t>(nblocks, 1)));
    for (size_t base = 0; base < nblocks; base += window) {
        const size_t n = std::min(window, nblocks - base);
        parallel_for(n, [&](size_t i) {
            std::string &o = piece[i];
            o.clear();
            o.reserve(BLOCK * (8 + 2 * dimensions * 20));
            char buf[512];
            const size_t lo = (base + i) * BLOCK, hi = std::min(num_nodes, lo + BLOCK);
            for (size_t node = lo; node < hi; ++node) {
                auto r = std::to_chars(buf, buf + sizeof buf, node);
                o.append(buf, r.ptr);
                for (size_t end = 0; end < 2; ++end)
                    for (size_t d = 0; d < dimensions; ++d) {
                        o.push_back('\t');
                        const double v = get(node, end, d);
                        if (v != v || std::isinf(v)) { o += rust_display_f64(v); continue; }
                        auto rv = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
                        o.append(buf, rv.ptr);
                    }
                o.push_back('\n');
            }
        });
        for (size_t i = 0; i < n; ++i) out.write(piece[i].data(), (std::streamsize)piece[i].size());
    }
}

// ---- SGD entry points ------------------------------------------------------------------------------
static void check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("gfasort_hip: ") + gfs_last_error());
}

// positions by dense index; empty when the reference returns an empty map
static std::vector<double> path_linear_sgd_vec(const BidirectedGraph &g, const FlatGraph &f, const PathSGDParams &p,
                                               const HipOptions &opt, gfs_stats *stats) {
    std::vector<double> x;
    if (g.node_count() == 0) return x;                               // sgd.rs:242-244
    gfs_graph_view v = f.view();
    gfs_sgd_params cp = p.to_c();
    x.resize(f.node_len.size());
    gfs_stats st;
    int rc = gfs_path_linear_sgd(&v, &cp, &opt.cfg, nullptr, nullptr, 1, x.data(), &st);
    check(rc);
    if (stats) *stats = st;
    if (rc == GFS_NOTHING_TO_DO) {
        std::cerr << "[path_sgd] No paths with multiple steps found\n";   // sgd.rs:259
        x.clear();
    }
    return x;
}

std::unordered_map<size_t, double> path_linear_sgd(const BidirectedGraph &g, const PathSGDParams &p,
                                                   const HipOptions &opt, gfs_stats *stats) {
    std::unordered_map<size_t, double> positions;
    FlatGraph f = g.flatten();
    std::vector<double> x = path_linear_sgd_vec(g, f, p, opt, stats);
    positions.reserve(x.size());
    for (size_t i = 0; i < x.size(); ++i) positions.emplace(i, x[i]);       // sgd.rs:604-607
    return positions;
}

namespace {
struct Lap {                                                        // GFS_TIMING=1: phase times on stderr
    bool on = std::getenv("GFS_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[sgd_sort] %-14s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};
}  // namespace

std::vector<Handle> path_sgd_sort(const BidirectedGraph &g, const PathSGDParams &p, const HipOptions &opt,
                                  gfs_stats *stats, std::vector<double> *positions_out) {
    if (positions_out) positions_out->clear();
    // same result as sorting path_linear_sgd's map (sgd.rs:641-672); the sort runs on the device
    std::vector<Handle> out;
    if (g.node_count() == 0) return out;                             // sgd.rs:242-244
    Lap lap;
    FlatGraph f = g.flatten();
    lap("flatten");
    gfs_graph_view v = f.view();
    gfs_sgd_params cp = p.to_c();
    std::vector<double> x(f.node_len.size());
    std::vector<uint64_t> order(x.size());
    gfs_stats st;
    int rc = gfs_path_sgd_sort(&v, &cp, &opt.cfg, nullptr, nullptr, 1, x.data(), order.data(), &st);
    lap("gfs_path_sgd_sort");
    check(rc);
    if (stats) *stats = st;
    if (rc == GFS_NOTHING_TO_DO) {
        std::cerr << "[path_sgd] No paths with multiple steps found\n";   // sgd.rs:259
        return out;
    }
    out.reserve(order.size());
    for (uint64_t idx : order) out.push_back(Handle::forward(f.node_ids[idx]));   // idx -> handle, sgd.rs:649-662
    lap("handles");
    if (positions_out) *positions_out = std::move(x);
    return out;
}

void sgd_sort_only(BidirectedGraph &g, const PathSGDParams &p, uint8_t verbose, const HipOptions &opt, gfs_stats *stats,
                   std::vector<double> *positions_out) {
    if (verbose >= 2) std::cerr << "[path_sgd] Starting path-guided SGD\n";
    auto ordering = path_sgd_sort(g, p, opt, stats, positions_out);
    Lap lap;
    g.apply_ordering(ordering);
    lap("apply_ordering");
    if (verbose >= 2) std::cerr << "[path_sgd] Complete\n";
}

// ---- batches: what sgd_sort_batch and sgd_layout_batch share ------------------------------------------------------------------
size_t refused_batch_item(int rc, const std::string &why, size_t n) {
    static const char phrase[] = "batch item ";
    const size_t at = why.find(phrase);
    const char *digits = at == std::string::npos ? "" : why.c_str() + at + sizeof phrase - 1;
    char *end = nullptr;
    const unsigned long long named = std::strtoull(digits, &end, 10);
    if (rc != GFS_E_UNSUPPORTED || end == digits || named >= n) throw std::runtime_error("gfasort_hip: " + why);
    return (size_t)named;
}

namespace {
struct Destroy {
    void operator()(gfs_ctx *c) const { gfs_ctx_destroy(c); }
    void operator()(gfs_batch *b) const { gfs_batch_destroy(b); }
    void operator()(gfs_ctx_set *s) const { gfs_ctx_set_destroy(s); }
};
using CtxHandle = std::unique_ptr<gfs_ctx, Destroy>;
using BatchHandle = std::unique_ptr<gfs_batch, Destroy>;     // borrows its contexts: declared after them, so that it goes first
// A graph on the device, and the flattened graph its context reads.  The context is its own, or an item of the drivers' context
// set: gfs_ctx_destroy leaves an item alone (it goes with its set), so the handle of an item owns nothing, and ctx.reset() on
// an item only lets go of it — its index arrays and what its setup allocated stay on the device until the set is destroyed at the
// end of the driver (graphs of fewer than SET_MAX_NODES nodes: a few hundred KB each), where a context of its own is freed at once.
// set_up: the item was set up with its set (gfs_ctx_set_setup_*), and rc is what its setup returned.
struct Slot { CtxHandle ctx; FlatGraph f; bool set_up = false; int rc = GFS_OK; };
using SetHandle = std::unique_ptr<gfs_ctx_set, Destroy>;     // owns its items: declared before the slots and the batch, so that it goes last
constexpr size_t SET_MAX_NODES = 16384;                       // graphs of fewer nodes are a batch's candidates under the default policy
}  // namespace

// The contexts of the graphs a batch can take — wanted(i), fewer than SET_MAX_NODES nodes, flags that ask for bundle 0 (auto) or
// 1 — built in ONE gfs_ctx_set instead of one gfs_ctx_create each (K3b), and set up in ONE pass instead of one gfs_ctx_setup_* each
// (K3c): setup_all(set, idx, item_rc) calls gfs_ctx_set_setup_1d / _nd with the parameters of the graphs idx, in item order.  Their
// slots are flattened, hold their item and what its setup returned; every other slot is left for open_slot.  Empty when no graph
// qualifies.
template <class Items, class Wanted, class SetupAll>
static SetHandle open_set(std::vector<Slot> &slots, const Items &items, const HipOptions &opt, uint8_t verbose, Wanted wanted, SetupAll setup_all) {
    const uint32_t bundle = (opt.cfg.flags >> 16) & 0xFFu;
    std::vector<size_t> idx;
    std::vector<gfs_graph_view> views;
    if (bundle > 1) return {};
    for (size_t i = 0; i < items.size(); ++i) {
        if (!items[i].graph || !wanted(i)) continue;
        const size_t n = items[i].graph->node_count();
        if (n == 0 || n >= SET_MAX_NODES) continue;
        slots[i].f = items[i].graph->flatten();
        idx.push_back(i);
        views.push_back(slots[i].f.view());
    }
    if (idx.empty()) return {};
    std::vector<const gfs_graph_view *> ptrs;
    for (const gfs_graph_view &v : views) ptrs.push_back(&v);
    gfs_ctx_set *s = nullptr;
    check(gfs_ctx_set_create(ptrs.data(), ptrs.size(), 0, &s));
    SetHandle set(s);
    if (verbose >= 2) {
        gfs_ctx_set_info info{};
        check(gfs_ctx_set_get_info(s, &info));
        std::cerr << "[gfasort_hip] batch: contexts of " << info.items << " graphs built together, " << info.build_ms << " ms, "
                  << info.launches << " launches\n";
    }
    std::vector<int32_t> rcs(idx.size(), GFS_OK);
    check(setup_all(s, idx, rcs.data()));
    if (verbose >= 2) {
        gfs_ctx_set_setup_info info{};
        check(gfs_ctx_set_get_setup_info(s, &info));
        std::cerr << "[gfasort_hip] batch: " << info.items << " graphs set up together, " << info.setup_ms << " ms, " << info.device_allocations
                  << " allocations, " << info.copies << " copies, " << info.launches << " launches\n";
    }
    // (last, after everything that can throw: a slot must never hold an item of a set that has already gone)
    for (size_t k = 0; k < idx.size(); ++k) {
        slots[idx[k]].ctx.reset(gfs_ctx_set_item(s, k));
        slots[idx[k]].set_up = true; slots[idx[k]].rc = rcs[k];
    }
    return set;
}

// Flatten g, create its context and set it up with setup(ctx), unless open_set has done all three.  Returns what the setup
// returned: on GFS_NOTHING_TO_DO the slot has let go of its context (a context of its own is destroyed, an item stays with its
// set), otherwise it is resident and `stats` says what it will run.
template <class Setup>
static int open_slot(Slot &s, const BidirectedGraph &g, gfs_stats &stats, Setup setup) {
    gfs_ctx *c = s.ctx.get();
    if (!c) {
        s.f = g.flatten();
        gfs_graph_view v = s.f.view();
        check(gfs_ctx_create(&v, 0, &c));
        s.ctx.reset(c);
    }
    const int rc = s.set_up ? s.rc : setup(c);                           // (a graph that runs alone keeps the single call)
    check(rc);
    if (rc == GFS_NOTHING_TO_DO) s.ctx.reset();
    else check(gfs_ctx_stats(c, &stats));
    return rc;
}

// One gfs_batch of the contexts of `together` (indices into slots).  A graph the batch refuses (flags that rule the fused launch
// out, more workgroups than one launch holds) is named by the error: it moves from `together` to `refused`, for the caller to
// run alone, and the others are tried again.  Empty when nothing is left.
static BatchHandle create_batch(const std::vector<Slot> &slots, std::vector<size_t> &together, std::vector<size_t> &refused, uint8_t verbose) {
    while (!together.empty()) {
        std::vector<gfs_ctx *> ctxs;
        for (size_t i : together) ctxs.push_back(slots[i].ctx.get());
        gfs_batch *b = nullptr;
        const int rc = gfs_batch_create(ctxs.data(), ctxs.size(), nullptr, &b);
        if (rc >= 0) return BatchHandle(b);
        const std::string why = gfs_last_error();
        const size_t named = refused_batch_item(rc, why, together.size());
        if (verbose >= 1) std::cerr << "[gfasort_hip] batch: graph " << together[named] << " runs alone (" << why << ")\n";
        refused.push_back(together[named]);
        together.erase(together.begin() + (std::ptrdiff_t)named);
    }
    return {};
}

// keep_profile: the pair errors of every item of a resident batch at its own step_distance_ladder, in ONE gfs_batch_pair_errors:
// the ladders are prefixes of the longest one (the rungs do not depend on the graph, only where they stop), so the longest is
// measured for all and every item keeps its own rungs.  together[k]: the graph of the batch's k-th item.
template <class Item>
static void batch_profiles(gfs_batch *b, const std::vector<Slot> &slots, std::vector<Item> &items, const std::vector<size_t> &together) {
    std::vector<std::vector<uint64_t>> ladders;
    size_t longest = 0;
    for (size_t i : together) {
        ladders.push_back(step_distance_ladder(slots[i].f));
        if (ladders.back().size() > ladders[longest].size()) longest = ladders.size() - 1;
    }
    const std::vector<uint64_t> &zs = ladders[longest];
    std::vector<gfs_pair_error> rows(together.size() * zs.size());
    check(gfs_batch_pair_errors(b, zs.data(), zs.size(), rows.data(), nullptr, nullptr));
    for (size_t k = 0; k < together.size(); ++k)
        items[together[k]].profile.assign(rows.begin() + (std::ptrdiff_t)(k * zs.size()), rows.begin() + (std::ptrdiff_t)(k * zs.size() + ladders[k].size()));
}

// diagnose_ratio >= 0: the diagnosis of every item of a resident batch at z = 1 and cap = 20, what layout_diagnosis gives one graph
// at a time from a fresh context: one gfs_batch_path_errors and one gfs_batch_stretched_pairs for all of them.
template <class Item>
static void batch_diagnoses(gfs_batch *b, std::vector<Item> &items, const std::vector<size_t> &together, double ratio, uint8_t verbose) {
    const uint64_t cap = 20;
    std::vector<uint64_t> offsets(together.size() + 1), totals(together.size());
    check(gfs_batch_path_offsets(b, offsets.data(), offsets.size()));
    std::vector<gfs_path_error> paths(offsets.back());
    std::vector<gfs_stretched_pair> pairs(together.size() * cap);
    check(gfs_batch_path_errors(b, 1, ratio, paths.data(), paths.size(), nullptr, nullptr));
    check(gfs_batch_stretched_pairs(b, 1, ratio, pairs.data(), cap, totals.data(), nullptr, nullptr));
    for (size_t k = 0; k < together.size(); ++k) {
        LayoutDiagnosis &d = items[together[k]].diagnosis;
        d.paths.assign(paths.begin() + (std::ptrdiff_t)offsets[k], paths.begin() + (std::ptrdiff_t)offsets[k + 1]);
        d.total = totals[k];
        d.pairs.assign(pairs.begin() + (std::ptrdiff_t)(k * cap), pairs.begin() + (std::ptrdiff_t)(k * cap + std::min<uint64_t>(cap, totals[k])));
    }
    if (verbose >= 1) std::cerr << "[gfasort_hip] batch: diagnosis of " << together.size() << " graphs read while resident\n";
}

// keep_sort_quality: gfs_ctx_sort_quality of every item of a resident batch of sorts, in ONE gfs_batch_sort_quality
static void batch_sort_qualities(gfs_batch *b, std::vector<BatchSortItem> &items, const std::vector<size_t> &together) {
    std::vector<gfs_sort_quality> rows(together.size());
    check(gfs_batch_sort_quality(b, rows.data(), rows.size(), nullptr, nullptr));
    for (size_t k = 0; k < together.size(); ++k) items[together[k]].quality = SortQuality::from_sums(rows[k]);
}

static void add_batch_stats(gfs_batch_stats &sum, const gfs_batch_stats &one) {
    sum.items += one.items; sum.items_run += one.items_run; sum.launches += one.launches; sum.blocks += one.blocks;
    sum.term_updates += one.term_updates; sum.attempts += one.attempts; sum.kernel_ms += one.kernel_ms; sum.total_ms += one.total_ms;
}

gfs_batch_stats sgd_sort_batch(std::vector<BatchSortItem> &items, uint8_t verbose, const HipOptions &opt, bool keep_positions, bool keep_profile,
                               double diagnose_ratio, bool keep_sort_quality) {
    SetHandle set;                                                                    // (outlives the slots and the batch)
    std::vector<Slot> slots(items.size());
    set = open_set(slots, items, opt, verbose, [](size_t) { return true; }, [&](gfs_ctx_set *s, const std::vector<size_t> &idx, int32_t *rcs) {
        std::vector<gfs_sgd_params> ps;
        for (size_t i : idx) ps.push_back(items[i].params.to_c());
        const std::vector<gfs_launch_config> cfgs(idx.size(), opt.cfg);
        return gfs_ctx_set_setup_1d(s, ps.data(), cfgs.data(), rcs);
    });
    gfs_batch_stats bs{};
    // reorder the graph by its rank order, keep what was asked for, free the context
    auto apply = [&](size_t i, std::vector<double> &&x, const auto *order, size_t n) {
        BatchSortItem &it = items[i];
        const FlatGraph &f = slots[i].f;
        check(gfs_ctx_stats(slots[i].ctx.get(), &it.stats));
        slots[i].ctx.reset();
        std::vector<Handle> ordering;
        ordering.reserve(n);
        for (size_t r = 0; r < n; ++r) ordering.push_back(Handle::forward(f.node_ids[order[r]]));   // idx -> handle, sgd.rs:649-662
        it.graph->apply_ordering(ordering);
        if (keep_positions) { it.positions = std::move(x); it.before = std::move(slots[i].f); }
    };
    // a graph that runs alone: start positions, run, read back through its own context
    auto finish_alone = [&](size_t i) {
        gfs_ctx *c = slots[i].ctx.get();
        check(gfs_ctx_init_positions(c));
        check(gfs_ctx_run(c, nullptr));
        std::vector<double> x(slots[i].f.node_len.size());
        std::vector<uint64_t> order(x.size());
        check(gfs_ctx_download_positions(c, x.data(), x.size()));
        check(gfs_ctx_sort_order(c, order.data(), order.size()));
        apply(i, std::move(x), order.data(), order.size());
    };
    std::vector<size_t> together, refused;                                            // indices into items: the batch's candidates
    for (size_t i = 0; i < items.size(); ++i) {
        BatchSortItem &it = items[i];
        it.stats = gfs_stats{}; it.batched = false; it.positions.clear(); it.profile.clear(); it.diagnosis = LayoutDiagnosis{};
        it.quality = SortQuality{};
        if (!it.graph || it.graph->node_count() == 0) continue;                       // sgd.rs:242-244
        const gfs_sgd_params cp = it.params.to_c();
        if (open_slot(slots[i], *it.graph, it.stats, [&](gfs_ctx *c) { return gfs_ctx_setup_1d(c, &cp, &opt.cfg, nullptr, nullptr); }) == GFS_NOTHING_TO_DO)
            std::cerr << "[path_sgd] No paths with multiple steps found\n";          // sgd.rs:259
        else if (it.stats.bundle == 1) together.push_back(i);                         // stays resident until the batch has run
        else finish_alone(i);                                                         // a team-kernel graph: alone, now
    }
    if (BatchHandle b = create_batch(slots, together, refused, verbose)) {
        // start positions, the run and the read-out of all its graphs: one launch each, two copies (K4b, K1f, K6b)
        check(gfs_batch_init_positions(b.get(), nullptr));
        check(gfs_batch_run(b.get(), nullptr));
        check(gfs_batch_get_stats(b.get(), &bs));
        std::vector<uint64_t> offsets(together.size() + 1);
        check(gfs_batch_result_offsets(b.get(), offsets.data(), offsets.size()));
        std::vector<double> x(offsets.back());
        std::vector<uint32_t> order(offsets.back());
        double readout_ms = 0.0;
        check(gfs_batch_results(b.get(), x.data(), order.data(), offsets.back(), &readout_ms, nullptr));
        if (verbose >= 2) std::cerr << "[gfasort_hip] batch: read-out of " << together.size() << " graphs, " << readout_ms << " ms on the device\n";
        if (keep_profile) batch_profiles(b.get(), slots, items, together);
        if (diagnose_ratio >= 0.0) batch_diagnoses(b.get(), items, together, diagnose_ratio, verbose);
        if (keep_sort_quality) batch_sort_qualities(b.get(), items, together);
        b.reset();                                                                    // (before its contexts go)
        for (size_t k = 0; k < together.size(); ++k) {
            items[together[k]].batched = true;
            apply(together[k], std::vector<double>(x.begin() + (std::ptrdiff_t)offsets[k], x.begin() + (std::ptrdiff_t)offsets[k + 1]),
                  order.data() + offsets[k], (size_t)(offsets[k + 1] - offsets[k]));
        }
    }
    for (size_t i : refused) finish_alone(i);
    return bs;
}

std::vector<double> default_layout_init(const FlatGraph &f, size_t D, uint64_t seed) {
    // the reference's own start (sgd.rs:829-853): dimension 0 = bp prefix, dimensions >= 1 = StandardNormal * sqrt(2N)
    // from one Xoshiro256+ seeded `seed` (gfs_init_layout restates rand_distr's ziggurat: parity unpinned)
    const size_t N = f.node_len.size(), n = N * 2 * D;
    std::vector<double> c(n, 0.0);
    gfs_graph_view v = f.view();
    gfs_init_layout(&v, D, seed, c.data());
    return c;
}

Layout path_linear_sgd_layout(const BidirectedGraph &g, const LayoutSGDParams &p, const HipOptions &opt, gfs_stats *stats) {
    size_t N = g.node_count();
    if (N == 0) return Layout(p.dimensions, 0);                      // sgd.rs:780-782
    FlatGraph f = g.flatten();
    gfs_graph_view v = f.view();
    gfs_layout_params cp = p.to_c();
    std::vector<double> coords = default_layout_init(f, p.dimensions, p.seed);
    gfs_stats st;
    int rc = gfs_path_linear_sgd_layout(&v, &cp, &opt.cfg, nullptr, nullptr, coords.data(), &st);
    check(rc);
    if (stats) *stats = st;
    if (rc == GFS_NOTHING_TO_DO) {
        std::cerr << "[path_sgd_layout] No paths with multiple steps found\n";   // sgd.rs:796
        return Layout(p.dimensions, N);
    }
    Layout l(p.dimensions, N);
    l.coords = std::move(coords);
    return l;
}

gfs_batch_stats sgd_layout_batch(std::vector<BatchLayoutItem> &items, uint8_t verbose, const HipOptions &opt, bool keep_profile, double diagnose_ratio) {
    SetHandle set;                                                                    // (outlives the slots and the batch)
    std::vector<Slot> slots(items.size());
    set = open_set(slots, items, opt, verbose, [&](size_t i) { return items[i].params.dimensions == 2 || items[i].params.dimensions == 3; },
                   [&](gfs_ctx_set *s, const std::vector<size_t> &idx, int32_t *rcs) {
        std::vector<gfs_layout_params> ps;
        for (size_t i : idx) ps.push_back(items[i].params.to_c());
        const std::vector<gfs_launch_config> cfgs(idx.size(), opt.cfg);
        return gfs_ctx_set_setup_nd(s, ps.data(), cfgs.data(), rcs);
    });
    gfs_batch_stats bs{};
    // a graph that runs alone: the single call, after the slot has let go of its context (an item of the set stays resident beside it)
    auto finish_alone = [&](size_t i) {
        slots[i].ctx.reset();
        items[i].layout = path_linear_sgd_layout(*items[i].graph, items[i].params, opt, &items[i].stats);
    };
    std::vector<size_t> candidates;                                                   // indices into items, of either dimension
    for (size_t i = 0; i < items.size(); ++i) {
        BatchLayoutItem &it = items[i];
        it.stats = gfs_stats{}; it.batched = false; it.profile.clear(); it.diagnosis = LayoutDiagnosis{};
        const size_t D = it.params.dimensions;
        it.layout = Layout(D, 0);
        if (!it.graph || it.graph->node_count() == 0) continue;                       // sgd.rs:780-782
        if (D != 2 && D != 3) { finish_alone(i); continue; }                          // no batch kernel for the dimension
        const gfs_layout_params cp = it.params.to_c();
        const int rc = open_slot(slots[i], *it.graph, it.stats, [&](gfs_ctx *c) { return gfs_ctx_setup_nd(c, &cp, &opt.cfg, nullptr, nullptr); });
        if (rc == GFS_NOTHING_TO_DO || it.stats.bundle != 1) { it.stats = gfs_stats{}; finish_alone(i); continue; }   // (the single call says why)
        candidates.push_back(i);                                                      // stays resident until its batch has run
    }
    for (size_t D : {(size_t)2, (size_t)3}) {
        std::vector<size_t> together, refused;
        for (size_t i : candidates) if (items[i].params.dimensions == D) together.push_back(i);
        if (BatchHandle b = create_batch(slots, together, refused, verbose)) {
            // start coordinates, the run and the read-out of all its graphs: one call each (K4c, K2f, K6c)
            std::vector<uint64_t> offsets(together.size() + 1);
            check(gfs_batch_result_offsets(b.get(), offsets.data(), offsets.size()));
            std::vector<double> coords(offsets.back() * 2 * D);
            for (size_t k = 0; k < together.size(); ++k) {
                const std::vector<double> c0 = default_layout_init(slots[together[k]].f, D, items[together[k]].params.seed);
                std::copy(c0.begin(), c0.end(), coords.begin() + (std::ptrdiff_t)(offsets[k] * 2 * D));
            }
            check(gfs_batch_upload_coords(b.get(), coords.data(), coords.size(), nullptr));
            check(gfs_batch_run(b.get(), nullptr));
            gfs_batch_stats one{};
            check(gfs_batch_get_stats(b.get(), &one));
            add_batch_stats(bs, one);
            double readout_ms = 0.0;
            check(gfs_batch_coords(b.get(), coords.data(), coords.size(), &readout_ms, nullptr));
            if (verbose >= 2) std::cerr << "[gfasort_hip] batch: coordinates of " << together.size() << " graphs, " << readout_ms << " ms on the device\n";
            if (keep_profile) batch_profiles(b.get(), slots, items, together);
            if (diagnose_ratio >= 0.0) batch_diagnoses(b.get(), items, together, diagnose_ratio, verbose);
            b.reset();                                                                // (before its contexts go)
            for (size_t k = 0; k < together.size(); ++k) {
                const size_t i = together[k];
                BatchLayoutItem &it = items[i];
                it.batched = true;
                check(gfs_ctx_stats(slots[i].ctx.get(), &it.stats));
                slots[i].ctx.reset();
                it.layout = Layout(D, slots[i].f.node_len.size());
                std::copy(coords.begin() + (std::ptrdiff_t)(offsets[k] * 2 * D), coords.begin() + (std::ptrdiff_t)(offsets[k + 1] * 2 * D), it.layout.coords.begin());
            }
        }
        for (size_t i : refused) finish_alone(i);
    }
    return bs;
}

// ---- calculate_layout_stress (sgd.rs:1196-1283) -----------------------------------------------------
double calculate_layout_stress(const BidirectedGraph &g, const Layout &layout, size_t sample_count) {
    FlatGraph f = g.flatten();
    const size_t S = f.step_node.size();
    if (S < 2) return 0.0;
    std::vector<uint64_t> pos(S);
    for (size_t p = 0; p + 1 < f.path_first_step.size(); ++p) {
        uint64_t position = 0;
        for (uint64_t s = f.path_first_step[p]; s < f.path_first_step[p + 1]; ++s) {
            pos[s] = position;
            if (f.step_node[s] != GFS_NO_NODE) position += f.node_len[f.step_node[s]];
        }
    }
    // the pairs: the library's restatement of the reference's draws (seed 12345; host only, no device needed)
    std::vector<uint64_t> step_a(sample_count), step_b(sample_count);
    uint64_t n_pairs = 0;
    gfs_graph_view v = f.view();
    check(gfs_stress_sample_pairs(&v, sample_count, 12345, step_a.data(), step_b.data(), &n_pairs));
    double sum = 0.0; uint64_t count = 0;
    for (uint64_t k = 0; k < n_pairs; ++k) {
        const uint64_t sa = step_a[k], sb = step_b[k];
        double path_dist = std::fabs((double)pos[sa] - (double)pos[sb]);
        if (path_dist == 0.0) continue;
        uint32_t ia = f.step_node[sa], ib = f.step_node[sb];
        if (ia == GFS_NO_NODE || ib == GFS_NO_NODE) continue;
        double err = layout.distance(ia, 0, ib, 0) - path_dist;
        sum += (err * err) / (path_dist * path_dist);
        ++count;
    }
    return count ? std::sqrt(sum / (double)count) : 0.0;
}

// ---- exhaustive per-step-distance errors on the device (gfs_pair_errors) ----------------------------------------------
std::vector<gfs_pair_error> layout_pair_errors(const FlatGraph &f, size_t dims, const std::vector<double> &positions,
                                               const std::vector<uint64_t> &zs) {
    const size_t want = dims ? f.node_len.size() * 2 * dims : f.node_len.size();
    if (positions.size() != want) throw std::runtime_error("layout_pair_errors: positions do not match the graph");
    std::vector<gfs_pair_error> out(zs.size());
    gfs_graph_view v = f.view();
    check(gfs_pair_errors(&v, dims, positions.data(), zs.data(), zs.size(), out.data()));
    return out;
}

SortQuality SortQuality::from_sums(const gfs_sort_quality &q) {
    SortQuality o;
    o.steps = q.steps; o.abs_err_sum = q.abs_err_sum; o.genomic_sum = q.genomic_sum; o.sq_err_sum = q.sq_err_sum;
    if (q.steps) {
        o.rmse = std::sqrt(q.sq_err_sum / (double)q.steps);
        o.mae = (double)q.abs_err_sum / (double)q.steps;
        if (q.genomic_sum) o.relative_error = o.mae / ((double)q.genomic_sum / (double)q.steps);
    }
    return o;
}

SortQuality sort_quality(const FlatGraph &f, const std::vector<double> &x) {
    if (x.size() != f.node_len.size()) throw std::runtime_error("sort_quality: positions do not match the graph");
    gfs_graph_view v = f.view();
    gfs_sort_quality q{};
    check(gfs_sort_quality_of(&v, x.data(), &q));
    return SortQuality::from_sums(q);
}

std::vector<gfs_pair_error> layout_pair_errors(const BidirectedGraph &g, const Layout &layout, const std::vector<uint64_t> &zs) {
    return layout_pair_errors(g.flatten(), layout.dimensions, layout.coords, zs);
}

std::vector<gfs_pair_error> layout_pair_errors(const BidirectedGraph &g, const std::vector<double> &positions,
                                               const std::vector<uint64_t> &zs) {
    return layout_pair_errors(g.flatten(), 0, positions, zs);
}

LayoutDiagnosis layout_diagnosis(const FlatGraph &f, size_t dims, const std::vector<double> &positions, uint64_t z, double ratio,
                                 uint64_t cap) {
    const size_t want = dims ? f.node_len.size() * 2 * dims : f.node_len.size();
    if (positions.size() != want) throw std::runtime_error("layout_diagnosis: positions do not match the graph");
    LayoutDiagnosis d;
    d.paths.resize(f.path_first_step.size() - 1);
    d.pairs.resize(cap);
    gfs_graph_view v = f.view();
    check(gfs_diagnose(&v, dims, positions.data(), z, ratio, d.paths.data(), cap ? d.pairs.data() : nullptr, cap, &d.total));
    d.pairs.resize(std::min<uint64_t>(cap, d.total));
    return d;
}

std::vector<uint64_t> step_distance_ladder(const FlatGraph &f) {
    uint64_t longest = 0;
    for (size_t p = 0; p + 1 < f.path_first_step.size(); ++p) longest = std::max(longest, f.path_first_step[p + 1] - f.path_first_step[p]);
    std::vector<uint64_t> zs;
    for (unsigned k = 0; k < 63 && (1ull << k) < longest; ++k) {
        zs.push_back(1ull << k);
        if (k >= 1 && (3ull << (k - 1)) < longest) zs.push_back(3ull << (k - 1));
    }
    return zs;
}

}  // namespace gfasort
