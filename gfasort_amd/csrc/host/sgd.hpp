// sgd.hpp — C++ host mirror of the reference's SGD entry points on top of libgfasort_hip.so.
//   PathSGDParams        src/sgd.rs:196-234       YgsParams        src/ygs.rs:16-93
//   LayoutSGDParams      src/sgd.rs:676-763       Layout           src/layout.rs:17-163
//   path_linear_sgd      src/sgd.rs:237           path_sgd_sort    src/sgd.rs:641
//   sgd_sort_only        src/ygs.rs:195           path_linear_sgd_layout  src/sgd.rs:773
//   calculate_layout_stress  src/sgd.rs:1196
//   layout_pair_errors   (no reference equivalent) the same per-pair error over ALL pairs at given step distances, on the device
//   layout_diagnosis     src/bin/sgd_diagnostics.rs: per path reverse steps and errors, the stretched pairs — of given positions, on the device
// Same names, argument meaning and empty-result behaviour as the Rust functions.
#pragma once
#include <cstdint>
#include <iosfwd>
#include <string>
#include <unordered_map>
#include <vector>

#include "graph.hpp"

namespace gfasort {

struct PathSGDParams {                     // defaults: sgd.rs:214-234
    uint64_t iter_max = 100;
    uint64_t iter_with_max_learning_rate = 0;
    uint64_t min_term_updates = 100;
    double delta = 0.0;
    double eps = 0.01;
    double eta_max = 100.0;
    double theta = 0.99;
    uint64_t space = 100;
    uint64_t space_max = 100;
    uint64_t space_quantization_step = 100;
    double cooling_start = 0.5;
    size_t nthreads = 1;
    bool progress = false;
    uint64_t seed = 9399220;
    gfs_sgd_params to_c() const;
};

struct LayoutSGDParams {                   // defaults: sgd.rs:709-729
    size_t dimensions = 2;
    uint64_t iter_max = 30;
    uint64_t iter_with_max_learning_rate = 0;
    uint64_t min_term_updates = 100;
    double delta = 0.0;
    double eps = 0.01;
    double eta_max = 100.0;
    double theta = 0.99;
    uint64_t space = 100;
    uint64_t space_max = 1000;
    uint64_t space_quantization_step = 100;
    double cooling_start = 0.5;
    size_t nthreads = 1;
    bool progress = false;
    uint64_t seed = 9399220;
    static LayoutSGDParams from_graph(const BidirectedGraph &g, size_t dimensions, size_t nthreads);  // sgd.rs:733
    gfs_layout_params to_c() const;
};

struct YgsParams {                         // ygs.rs:16-45
    PathSGDParams path_sgd;
    uint8_t verbose = 0;
    YgsParams();
    static YgsParams from_graph(const BidirectedGraph &g, uint8_t verbose, size_t nthreads);          // ygs.rs:50
};

struct Layout {                            // layout.rs:17-24
    size_t dimensions = 0;
    size_t num_nodes = 0;
    std::vector<double> coords;            // coords[node*2*D + end*D + dim]
    Layout() = default;
    Layout(size_t dims, size_t n) : dimensions(dims), num_nodes(n), coords(n * 2 * dims, 0.0) {}
    static Layout from_vectors(const std::vector<std::vector<double>> &coord_vecs);                   // layout.rs:39
    size_t index(size_t node, size_t end, size_t dim) const { return node * 2 * dimensions + end * dimensions + dim; }
    double get(size_t node, size_t end, size_t dim) const { return coords[index(node, end, dim)]; }
    void set(size_t node, size_t end, size_t dim, double v) { coords[index(node, end, dim)] = v; }
    double distance(size_t na, size_t ea, size_t nb, size_t eb) const;                                // layout.rs:126
    void write_tsv(std::ostream &out) const;                                                          // layout.rs:138
};

std::string rust_display_f64(double v);    // Rust `{}` on f64

// Device launch shape for the HIP engine (no reference equivalent; all-zero = defaults).
struct HipOptions {
    gfs_launch_config cfg{};
};

// sgd.rs:237 — dense index (position in node_order) -> final position; EMPTY when the reference
// returns an empty map.  Throws std::runtime_error on a HIP / argument error.
std::unordered_map<size_t, double> path_linear_sgd(const BidirectedGraph &g, const PathSGDParams &p,
                                                   const HipOptions &opt = {}, gfs_stats *stats = nullptr);
// sgd.rs:641 — handles in ascending position order (ties keep node_order; the reference's tie
// order is HashMap-random).
// positions_out (nullable): the final positions by dense index of g as it is BEFORE the ordering is applied; empty when
// there was nothing to do.
std::vector<Handle> path_sgd_sort(const BidirectedGraph &g, const PathSGDParams &p, const HipOptions &opt = {},
                                  gfs_stats *stats = nullptr, std::vector<double> *positions_out = nullptr);
// ygs.rs:195 — path_sgd_sort + apply_ordering.
void sgd_sort_only(BidirectedGraph &g, const PathSGDParams &p, uint8_t verbose, const HipOptions &opt = {},
                   gfs_stats *stats = nullptr, std::vector<double> *positions_out = nullptr);
// Which paths and pairs carry the error at step distance z (gfs_diagnose): one gfs_path_error per path, and the first `cap` of the
// pairs (s, s + z) whose layout distance is more than `ratio` times their path distance, in step order, with their exact total.
struct LayoutDiagnosis {
    std::vector<gfs_path_error> paths;
    std::vector<gfs_stretched_pair> pairs;
    uint64_t total = 0;
};
// measure_layout_quality.rs:100-208 for a sort's positions (gfs_sort_quality): the four sums, and the figures the reference derives
// from them (:162-208) — mse = sq_err_sum / steps, rmse = sqrt(mse), mae = abs_err_sum / steps, relative_error = mae / (genomic_sum /
// steps), each one double operation on exact inputs; zeros without a counted step.
struct SortQuality {
    uint64_t steps = 0, abs_err_sum = 0, genomic_sum = 0;
    double sq_err_sum = 0.0, rmse = 0.0, mae = 0.0, relative_error = 0.0;
    static SortQuality from_sums(const gfs_sort_quality &q);
};
// sgd_sort_only over MANY graphs (no reference equivalent; gfasort_hip --batch).  Graphs for which the policy picks reference streams
// (fewer than 16384 nodes) run together as one gfs_batch — one persistent launch, or as few as fit the device —, the others alone,
// one after the other; every graph is then reordered exactly as sgd_sort_only reorders it.  A graph that gfs_batch_create refuses
// (its error names the item) is taken out and runs alone; the rest still run together.  Only the batch's graphs are resident on
// the device at once: a graph that runs alone for its bundle is run, read back and freed before the next one is set up.
struct BatchSortItem {
    BidirectedGraph *graph = nullptr;      // reordered in place
    PathSGDParams params;
    gfs_stats stats{};                     // the graph's own (a batched graph's kernel_ms is the batch's: 0 here)
    bool batched = false;
    FlatGraph before;                      // keep_positions: the graph as it was flattened before the sort ...
    std::vector<double> positions;         // ... and the final positions by its dense index; empty where there was nothing to do
    std::vector<gfs_pair_error> profile;   // keep_profile, batched graphs: layout_pair_errors at step_distance_ladder, read while resident
    LayoutDiagnosis diagnosis;             // diagnose_ratio >= 0, batched graphs: layout_diagnosis(before, 0, positions, 1, ratio, 20), read while resident
    SortQuality quality;                   // keep_sort_quality, batched graphs: sort_quality(before, positions), read while resident
};
// Returns the batch's figures (all zero where no graph was batched).  Throws std::runtime_error on a HIP / argument error.
// keep_profile: the batched graphs' pair errors at their step_distance_ladder are read from the batch while it is resident
// (gfs_batch_pair_errors: one call for all of them), the figures layout_pair_errors gives for the kept positions.
// diagnose_ratio >= 0 (either driver): the batched graphs' diagnosis at z = 1, that ratio and cap = 20 is read from the batch while it
// is resident (gfs_batch_path_errors, gfs_batch_stretched_pairs: one call each for all of them), what layout_diagnosis gives for the
// final positions; negative: not asked for.
// keep_sort_quality: the batched graphs' sort quality is read from the batch while it is resident (gfs_batch_sort_quality: one call for
// all of them), what sort_quality gives for the kept positions.
gfs_batch_stats sgd_sort_batch(std::vector<BatchSortItem> &items, uint8_t verbose, const HipOptions &opt = {}, bool keep_positions = false,
                               bool keep_profile = false, double diagnose_ratio = -1.0, bool keep_sort_quality = false);
// path_linear_sgd_layout over MANY graphs (no reference equivalent; gfasort_hip --batch -p L), the layout twin of sgd_sort_batch.
// Every graph gets its own parameters and its own default_layout_init.  Graphs of 2 or 3 dimensions for which the policy picks
// the pooled reference-stream kernel (stats.bundle == 1) run together, one gfs_batch per dimension: all start coordinates up
// in one call, one persistent launch (or as few as fit the device), all final coordinates down in one call.  The others —
// 4 to 8 dimensions, a team-kernel graph, a graph gfs_batch_create refuses (its error names the item) — run alone through
// path_linear_sgd_layout.  Every Layout is what the single run returns.
struct BatchLayoutItem {
    const BidirectedGraph *graph = nullptr;
    LayoutSGDParams params;
    Layout layout;                         // what path_linear_sgd_layout returns for the graph
    gfs_stats stats{};                     // the graph's own (a batched graph's kernel_ms is the batch's: 0 here)
    bool batched = false;
    std::vector<gfs_pair_error> profile;   // keep_profile, batched graphs: as BatchSortItem::profile, of the final coordinates
    LayoutDiagnosis diagnosis;             // diagnose_ratio >= 0, batched graphs: as BatchSortItem::diagnosis, of the final coordinates
};
// Returns the batches' figures, summed where both dimensions had one (all zero where no graph was batched).
gfs_batch_stats sgd_layout_batch(std::vector<BatchLayoutItem> &items, uint8_t verbose, const HipOptions &opt = {}, bool keep_profile = false,
                                 double diagnose_ratio = -1.0);
// Which of the n contexts handed to gfs_batch_create its refusal names: rc is what the call returned and why its
// gfs_last_error(), which reads "batch item K: ..." for a GFS_E_UNSUPPORTED.  Any other code, a text that names no item and a K
// outside [0, n) are the library's error as it stands: thrown as std::runtime_error.  Both batch drivers read refusals through
// this; it needs no device (host_selftest).
size_t refused_batch_item(int rc, const std::string &why, size_t n);
// sgd.rs:773.  Gaussian start of dims >= 1 is drawn here (Box-Muller on SplitMix64(seed); the
// reference's rand_distr ziggurat stream is not reproduced).
Layout path_linear_sgd_layout(const BidirectedGraph &g, const LayoutSGDParams &p, const HipOptions &opt = {},
                              gfs_stats *stats = nullptr);
std::vector<double> default_layout_init(const FlatGraph &f, size_t dims, uint64_t seed);
// sgd.rs:1196 (host, seed 12345)
double calculate_layout_stress(const BidirectedGraph &g, const Layout &layout, size_t sample_count);

// The error of calculate_layout_stress' formula over ALL pairs of path steps (s, s + z), one entry per step distance z, computed
// on the device (gfs_pair_errors): exhaustive and deterministic, no sample.  dims = 0: positions is x by dense index (a sort's
// result); otherwise Layout.coords.  Throws std::runtime_error on a HIP / argument error.
std::vector<gfs_pair_error> layout_pair_errors(const FlatGraph &f, size_t dims, const std::vector<double> &positions,
                                               const std::vector<uint64_t> &zs);
std::vector<gfs_pair_error> layout_pair_errors(const BidirectedGraph &g, const Layout &layout, const std::vector<uint64_t> &zs);
std::vector<gfs_pair_error> layout_pair_errors(const BidirectedGraph &g, const std::vector<double> &positions,
                                               const std::vector<uint64_t> &zs);
LayoutDiagnosis layout_diagnosis(const FlatGraph &f, size_t dims, const std::vector<double> &positions, uint64_t z = 1,
                                 double ratio = 10.0, uint64_t cap = 20);
// How good a sort is as a sort (gfs_sort_quality_of): x by dense index of f, measured on the device.  Throws as layout_pair_errors.
SortQuality sort_quality(const FlatGraph &f, const std::vector<double> &x);
// z = 1, 2, 3, 4, 6, 8, 12, 16, ...: every 2^k and 3 * 2^(k-1) below the longest path's step count
std::vector<uint64_t> step_distance_ladder(const FlatGraph &f);

}  // namespace gfasort
