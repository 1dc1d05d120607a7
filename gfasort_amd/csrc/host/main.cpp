// gfasort_hip — CLI with the flag surface of the reference binary (src/bin/gfasort.rs:49-86),
// running the `Y` (path-guided SGD sort) and `L` (nD layout) pipeline steps on the MI355X
// engine.  The other pipeline characters (g, s, S, u) belong to subsystems that are out of
// scope for this build: they are rejected with a clear message.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "sgd.hpp"

using namespace gfasort;

struct Args {
    std::string input, output, pipeline = "sYgs", layout_out;
    std::string layout_option;                     // the last of --dimensions / --layout-out / --layout-iter given: -p L only
    std::string batch_list;                        // --batch: a file of in.gfa<TAB>out.gfa[<TAB>layout.tsv] lines, all run in one invocation
    size_t iter_max = 100, threads = 1, dimensions = 2, layout_iter = 30;
    unsigned verbose = 1;
    uint64_t streams = 0; uint32_t flags = 0;      // HIP launch shape (extra, not in the reference)
    unsigned bundle = 0;                           // 0 = auto, 1 = reference streams, 4..64
    bool reference_sampler = false, phased = false;
    bool stress_profile = false;                   // after a Y or an L step: the exhaustive error per step distance
    bool diagnose = false;                         // after a Y or an L step: errors per path and the stretched adjacent pairs
    double diagnose_ratio = 10.0;
    bool sort_quality = false;                     // after a Y step: measure_layout_quality's figures for the sorted graph
};

static void usage() {
    std::cerr <<
        "Usage: gfasort_hip -i <in.gfa> -o <out.gfa> [-p PIPELINE] [--iter-max N] [-t N] [-v N]\n"
        "                   [--dimensions D] [--layout-out FILE] [--layout-iter N] [--streams N]\n"
        "                   [--io-threads N]   (host threads for GFA text passes; default: available CPUs, <= 16)\n"
        "                   [--bundle auto|1|4|8|16|32|64]   (sampling bundle; 1 = reference streams; 4: -p Y only;\n"
        "                                   auto gives --dimensions 4..8 reference streams, 8..64 their team kernels)\n"
        "                   [--reference-sampler]   (= --bundle 1: every term sampled independently, as src/sgd.rs:444-497 does;\n"
        "                                            ~8x slower on large graphs.  The default on graphs of >= 16384 nodes samples RUNS of\n"
        "                                            terms; on graphs whose haplotypes differ by kilobases it needs a longer schedule\n"
        "                                            (--iter-max 300) to reach what the reference's sampler reaches, DESIGN.md)\n"
        "                   [--phased-sampler]   (-p Y: the default sampler, but every term of a window of iterations around the\n"
        "                                       switch to the cooling phase sampled independently as --reference-sampler does;\n"
        "                                       reaches the reference's quality at the default --iter-max in ~half the time\n"
        "                                       of --reference-sampler.  Not with --reference-sampler or a --bundle other than\n"
        "                                       auto or 64; -p L is not affected.  -v 2 prints the window)\n"
        "                   [--stress-profile]   (after every Y or L step, on stderr: the error of ALL pairs of path steps z apart,\n"
        "                                       one line per step distance z = 1, 2, 3, 4, 6, 8, 12, ... — exhaustive, computed on\n"
        "                                       the device from the step's final positions; the sampled `layout stress` of -v is\n"
        "                                       dominated by the few short-range pairs it happens to hit)\n"
        "                   [--diagnose] [--diagnose-ratio R]   (after every Y or L step, on stderr, for adjacent path steps: per path\n"
        "                                       its steps, forward and reverse steps, counted pairs, rms relative error and stretched\n"
        "                                       pairs, then the first 20 stretched pairs — those whose layout distance is more than\n"
        "                                       R (default 10) times their path distance; computed on the device)\n"
        "                   [--sort-quality]   (after every Y step, on stderr: the figures of the reference's measure_layout_quality for\n"
        "                                     the graph as the step sorted it — counted steps, the sums of absolute error and of genomic\n"
        "                                     distance, rmse, mae and relative error in bp; computed on the device, all integers but\n"
        "                                     one sum added in a fixed order.  Refused for a pipeline without a Y step)\n"
        "       gfasort_hip --batch LIST -p Y [the options above, except -i, -o and those of -p L]\n"
        "                   (LIST: one in.gfa<TAB>out.gfa per line; every graph is sorted as a -i/-o run sorts it, the small ones —\n"
        "                    those that run reference streams — together in one persistent launch that fills the device, the\n"
        "                    others alone)\n"
        "       gfasort_hip --batch LIST -p L [the options above, except -i, -o, --layout-out and those of -p Y]\n"
        "                   (LIST: one in.gfa<TAB>out.gfa<TAB>layout.tsv per line; every graph is laid out as a -i/-o/--layout-out run\n"
        "                    lays it out, the small ones of 2 or 3 dimensions together in one persistent launch, the others alone.\n"
        "                    With --stress-profile or --diagnose either kind of batch, and with --sort-quality a batch of sorts, measures its\n"
        "                    graphs while they are resident)\n"
        "Pipeline characters: Y = path-guided SGD sort, L = nD layout (HIP engine).\n"
        "g, s, S, u exist in the reference but are not part of this build.\n";
}

static bool parse_args(int argc, char **argv, Args &a) {
    auto need = [&](int &i) -> const char * { if (i + 1 >= argc) { std::cerr << "error: missing value for " << argv[i] << "\n"; return nullptr; } return argv[++i]; };
    for (int i = 1; i < argc; ++i) {
        std::string f = argv[i];
        const char *v;
        if (f == "-i" || f == "--input") { if (!(v = need(i))) return false; a.input = v; }
        else if (f == "-o" || f == "--output") { if (!(v = need(i))) return false; a.output = v; }
        else if (f == "--batch") { if (!(v = need(i))) return false; a.batch_list = v; }
        else if (f == "-p" || f == "--pipeline") { if (!(v = need(i))) return false; a.pipeline = v; }
        else if (f == "--iter-max") { if (!(v = need(i))) return false; a.iter_max = std::stoull(v); }
        else if (f == "-t" || f == "--threads") { if (!(v = need(i))) return false; a.threads = std::stoull(v); }
        else if (f == "-v" || f == "--verbose") { if (!(v = need(i))) return false; a.verbose = (unsigned)std::stoul(v); }
        else if (f == "--dimensions") { if (!(v = need(i))) return false; a.dimensions = std::stoull(v); a.layout_option = f; }
        else if (f == "--layout-out") { if (!(v = need(i))) return false; a.layout_out = v; a.layout_option = f; }
        else if (f == "--layout-iter") { if (!(v = need(i))) return false; a.layout_iter = std::stoull(v); a.layout_option = f; }
        else if (f == "--io-threads") { if (!(v = need(i))) return false; set_io_threads(std::stoull(v)); }
        else if (f == "--streams") { if (!(v = need(i))) return false; a.streams = std::stoull(v); }
        else if (f == "--bundle") { if (!(v = need(i))) return false; a.bundle = std::string(v) == "auto" ? 0u : (unsigned)std::stoul(v); }
        else if (f == "--reference-sampler") { a.bundle = 1; a.reference_sampler = true; }
        else if (f == "--phased-sampler") { a.phased = true; }
        else if (f == "--stress-profile") { a.stress_profile = true; }
        else if (f == "--diagnose") { a.diagnose = true; }
        else if (f == "--sort-quality") { a.sort_quality = true; }
        else if (f == "--diagnose-ratio") { if (!(v = need(i))) return false; a.diagnose_ratio = std::stod(v); }
        else if (f == "--hip-flags") { if (!(v = need(i))) return false; a.flags = (uint32_t)std::stoul(v); }
        else if (f == "-h" || f == "--help") { usage(); exit(0); }
        else { std::cerr << "error: unexpected argument '" << f << "'\n"; return false; }
    }
    if (a.phased && (a.reference_sampler || (a.bundle != 0 && a.bundle != 64))) {
        std::cerr << "error: --phased-sampler switches between the reference sampler and bundles of 64: not with --reference-sampler or --bundle "
                  << a.bundle << "\n";
        return false;
    }
    if (a.sort_quality && a.pipeline.find('Y') == std::string::npos) {
        std::cerr << "error: --sort-quality measures the graph as a Y step sorted it: -p " << a.pipeline << " has no Y step\n";
        return false;
    }
    if (!a.batch_list.empty()) {
        if (!a.input.empty() || !a.output.empty()) { std::cerr << "error: --batch takes its inputs and outputs from LIST: not with -i / -o\n"; return false; }
        if (a.pipeline != "Y" && a.pipeline != "L") {
            std::cerr << "error: --batch runs one step over many graphs in one launch: it needs -p Y or -p L exactly, not -p " << a.pipeline << "\n";
            return false;
        }
        if (a.pipeline == "Y" && !a.layout_option.empty()) { std::cerr << "error: --batch sorts (-p Y): " << a.layout_option << " belongs to -p L\n"; return false; }
        if (a.pipeline == "L" && !a.layout_out.empty()) {
            std::cerr << "error: --batch -p L takes its layout files from LIST (in.gfa<TAB>out.gfa<TAB>layout.tsv): not with --layout-out\n";
            return false;
        }
        if (a.pipeline == "L" && a.phased) { std::cerr << "error: --batch lays out (-p L): --phased-sampler belongs to -p Y\n"; return false; }
        return true;
    }
    if (a.input.empty() || a.output.empty()) { std::cerr << "error: -i and -o are required\n"; return false; }
    return true;
}

static int validate_pipeline(const std::string &p) {                  // gfasort.rs:169-180
    for (char c : p) {
        switch (c) {
            case 'Y': case 'L': break;
            case 'g': case 's': case 'S': case 'u':
                std::cerr << "Error: pipeline step '" << c << "' is part of the reference but not of this build "
                             "(only Y = SGD and L = layout run on the HIP engine)\n";
                return 1;
            default:
                std::cerr << "Error: Unknown pipeline character '" << c
                          << "'. Valid: Y (SGD), g (groom), s (topo-sort), S (priority-topo-sort), u (unchop), L (layout)\n";
                return 1;
        }
    }
    if (p.empty()) { std::cerr << "Error: Pipeline cannot be empty\n"; return 1; }
    return 0;
}

static void print_stress_profile(const std::vector<gfs_pair_error> &rows) {
    for (const gfs_pair_error &r : rows) {
        const double n = (double)r.pairs;
        char buf[320];
        snprintf(buf, sizeof buf, "[gfasort] stress profile: z=%llu pairs=%llu rms_rel=%.17g max_rel=%.17g rmse_bp=%.17g mae_bp=%.17g\n",
                 (unsigned long long)r.step_distance, (unsigned long long)r.pairs, r.pairs ? std::sqrt(r.sum_rel_sq / n) : 0.0,
                 std::sqrt(r.max_rel_sq), r.pairs ? std::sqrt(r.sum_sq / n) : 0.0, r.pairs ? r.sum_abs / n : 0.0);
        std::cerr << buf;
    }
}

// The report of the reference's sgd_diagnostics binary, for the positions a step ended with: z = 1.  f: the graph the positions
// speak of (dense index); names: its paths'.  resident: the diagnosis, where a batch read it while the graph was resident.
static void print_diagnosis(const FlatGraph &f, const std::vector<BiPath> &paths, size_t dims, const std::vector<double> &positions,
                            double ratio, const LayoutDiagnosis *resident = nullptr) {
    const LayoutDiagnosis d = resident ? *resident : layout_diagnosis(f, dims, positions, 1, ratio, 20);
    char buf[512];
    std::cerr << "[gfasort] diagnosis: path orientation and adjacent-step errors\n";
    for (size_t p = 0; p < d.paths.size(); ++p) {
        const gfs_path_error &r = d.paths[p];
        snprintf(buf, sizeof buf, "[gfasort] diagnosis:   %s: %llu steps, %llu forward, %llu reverse (%.1f%% reverse), %llu pairs, "
                 "rms relative error %.6g, %llu stretched\n", p < paths.size() ? paths[p].name.c_str() : "?", (unsigned long long)r.steps,
                 (unsigned long long)(r.steps - r.reverse_steps), (unsigned long long)r.reverse_steps,
                 r.steps ? 100.0 * (double)r.reverse_steps / (double)r.steps : 0.0, (unsigned long long)r.pairs,
                 r.pairs ? std::sqrt(r.sum_rel_sq / (double)r.pairs) : 0.0, (unsigned long long)r.stretched);
        std::cerr << buf;
    }
    snprintf(buf, sizeof buf, "[gfasort] diagnosis: %llu adjacent pairs with layout distance > %g x path distance%s\n",
             (unsigned long long)d.total, ratio, d.total > d.pairs.size() ? " (the first 20 follow)" : "");
    std::cerr << buf;
    auto handle = [&](uint64_t s) {
        const uint32_t n = f.step_node[s];
        return (n == GFS_NO_NODE ? std::string("?") : std::to_string(f.node_ids[n])) + (f.step_is_rev[s] ? "-" : "+");
    };
    auto bp = [&](const gfs_stretched_pair &q, uint64_t s) {             // bp position of step s inside its path
        uint64_t pos = 0;
        for (uint64_t k = f.path_first_step[q.path]; k < s; ++k) if (f.step_node[k] != GFS_NO_NODE) pos += f.node_len[f.step_node[k]];
        return pos;
    };
    auto where = [&](uint64_t s) {                                       // the + end of the step's node
        const size_t n = f.step_node[s];
        std::string out;
        for (size_t k = 0; k < (dims ? dims : 1); ++k) {
            snprintf(buf, sizeof buf, "%s%.0f", k ? "," : "", positions[dims ? n * 2 * dims + k : n]);
            out += buf;
        }
        return out;
    };
    for (const gfs_stretched_pair &q : d.pairs) {
        const std::string name = q.path < paths.size() ? paths[q.path].name : "?";
        snprintf(buf, sizeof buf, "[gfasort] diagnosis:   %s %s->%s: path positions %llu -> %llu (dist=%.0fbp), layout positions %s -> %s "
                 "(dist=%.0f), ratio %.1fx\n", name.c_str(), handle(q.step_a).c_str(), handle(q.step_b).c_str(),
                 (unsigned long long)bp(q, q.step_a), (unsigned long long)bp(q, q.step_b), q.d_path, where(q.step_a).c_str(),
                 where(q.step_b).c_str(), q.d_layout, q.d_layout / q.d_path);
        std::cerr << buf;
    }
}

static void print_run_stats(const gfs_stats &st) {
    std::cerr << "[gfasort_hip] " << st.term_updates << " term updates in " << st.iterations << " iterations on "
              << st.n_streams << " streams (bundle " << st.bundle << "); kernels " << st.kernel_ms << " ms ("
              << (st.kernel_ms > 0 ? (double)st.term_updates / st.kernel_ms / 1e6 : 0.0) << " G updates/s), call "
              << st.total_ms << " ms\n";
}

// One column more than a sort's list: where the graph's layout goes.
struct BatchFiles { std::string in, out, layout; };

// The lines of LIST: in.gfa<TAB>out.gfa under -p Y, in.gfa<TAB>out.gfa<TAB>layout.tsv under -p L.  Needs no device.
static bool read_batch_list(const Args &args, bool layouts, std::vector<BatchFiles> &files) {
    std::ifstream list(args.batch_list);
    if (!list) { std::cerr << "Error reading file: " << args.batch_list << ": " << std::strerror(errno) << "\n"; return false; }
    std::string line;
    size_t n = 0;
    while (std::getline(list, line)) {
        ++n;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        std::vector<std::string> cols;
        size_t from = 0;
        for (size_t tab; (tab = line.find('\t', from)) != std::string::npos; from = tab + 1) cols.push_back(line.substr(from, tab - from));
        cols.push_back(line.substr(from));
        bool ok = cols.size() == (layouts ? 3u : 2u);
        for (const std::string &c : cols) ok = ok && !c.empty();
        if (!ok) {
            std::cerr << "Error: " << args.batch_list << " line " << n << ": expected "
                      << (layouts ? "in.gfa<TAB>out.gfa<TAB>layout.tsv (--batch -p L; two columns are a -p Y list)" : "in.gfa<TAB>out.gfa") << "\n";
            return false;
        }
        files.push_back(BatchFiles{cols[0], cols[1], layouts ? cols[2] : std::string()});
    }
    if (files.empty()) { std::cerr << "Error: " << args.batch_list << " lists no graph\n"; return false; }
    return true;
}

static void print_batch_stats(const gfs_batch_stats &bs) {
    std::cerr << "[gfasort_hip] batch: " << bs.items_run << " graphs in " << bs.launches << (bs.launches == 1 ? " launch" : " launches")
              << " of " << bs.blocks << " workgroups; kernels " << bs.kernel_ms << " ms ("
              << (bs.kernel_ms > 0 ? (double)bs.term_updates / bs.kernel_ms / 1e6 : 0.0) << " G updates/s), run " << bs.total_ms << " ms\n";
}

// --sort-quality: one line, every figure an integer or a double derived from integers and one sum of a fixed order (SortQuality)
static void print_sort_quality(const SortQuality &q) {
    char buf[256];
    snprintf(buf, sizeof buf, "steps=%llu abs_err_sum=%llu genomic_sum=%llu rmse_bp=%.17g mae_bp=%.17g relative_error=%.17g", (unsigned long long)q.steps,
             (unsigned long long)q.abs_err_sum, (unsigned long long)q.genomic_sum, q.rmse, q.mae, q.relative_error);
    std::cerr << "[gfasort] sort quality: " << buf << "\n";
}

// --stress-profile and --diagnose of the positions a step ended with: x by dense index of f (dims = 0, a sort; f is the graph as
// it was before the sort reordered it) or Layout.coords.  resident, resident_diagnosis: the profile and the diagnosis, where a batch
// read them while the graph was resident.  --sort-quality (sorts only) likewise, resident_quality.
static void print_measures(const Args &args, const FlatGraph &f, const std::vector<BiPath> &paths, size_t dims, const std::vector<double> &x,
                           const std::vector<gfs_pair_error> *resident = nullptr, const LayoutDiagnosis *resident_diagnosis = nullptr,
                           const SortQuality *resident_quality = nullptr) {
    if (args.stress_profile) print_stress_profile(resident ? *resident : layout_pair_errors(f, dims, x, step_distance_ladder(f)));
    if (args.diagnose) print_diagnosis(f, paths, dims, x, args.diagnose_ratio, resident_diagnosis);
    if (args.sort_quality && dims == 0) print_sort_quality(resident_quality ? *resident_quality : sort_quality(f, x));
}

static void print_layout_stress(const BidirectedGraph &g, const Layout &layout) {
    char buf[64]; snprintf(buf, sizeof buf, "%.6f", calculate_layout_stress(g, layout, 10000));
    std::cerr << "[gfasort] layout stress: " << buf << "\n";
}

// Every output file is written here: body(stream), closed, and an error of either said on stderr with the site's own words.
template <class Body>
static bool write_file(const std::string &path, const char *cannot_open, const char *cannot_write, Body body) {
    std::ofstream f(path, std::ios::binary);
    if (!f) { std::cerr << cannot_open << ": " << std::strerror(errno) << "\n"; return false; }
    body(f);
    f.close();                                                                        // (a full disk shows here at the latest)
    if (!f) { std::cerr << cannot_write << " " << path << ": " << std::strerror(errno) << "\n"; return false; }
    return true;
}

static bool write_gfa_file(const Args &args, const std::string &path, const BidirectedGraph &g) {
    if (args.verbose >= 1) std::cerr << "[gfasort] writing " << path << "\n";
    return write_file(path, "Error writing output file", "Error writing output file", [&](std::ostream &f) { g.write_gfa(f); });
}

static bool write_layout_file(const Args &args, const std::string &path, const Layout &layout) {
    if (args.verbose >= 1) std::cerr << "[gfasort] writing layout to " << path << "\n";
    return write_file(path, "Error creating layout file", "Error writing layout file", [&](std::ostream &f) { layout.write_tsv(f); });
}

// joins the warm-up thread on every way out that returns
struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } };

// --batch LIST: every graph of the list gets its own YgsParams::from_graph (-p Y) or LayoutSGDParams::from_graph (-p L), as a
// -i/-o run gives it; those that run reference streams (-p L: in 2 or 3 dimensions) go through the step in one batch, the others
// alone; every output is what the single run writes.
static int run_batch(const Args &args) {
    const bool layouts = args.pipeline == "L";
    std::vector<BatchFiles> files;
    if (!read_batch_list(args, layouts, files)) return 1;
    std::thread warm([] { (void)gfs_warmup(0); });
    Joiner joiner{warm};
    std::vector<BidirectedGraph> graphs(files.size());
    for (size_t i = 0; i < files.size(); ++i) {
        if (args.verbose >= 1) std::cerr << "[gfasort] reading " << files[i].in << "\n";
        try { graphs[i] = parse_gfa(read_file(files[i].in)); }
        catch (const std::exception &e) { std::cerr << "Error reading " << files[i].in << ": " << e.what() << "\n"; return 1; }
    }
    std::vector<BatchSortItem> sorts(layouts ? 0 : files.size());
    std::vector<BatchLayoutItem> lays(layouts ? files.size() : 0);
    for (size_t i = 0; i < sorts.size(); ++i) {
        sorts[i].graph = &graphs[i];
        sorts[i].params = YgsParams::from_graph(graphs[i], (uint8_t)args.verbose, args.threads).path_sgd;
        sorts[i].params.iter_max = args.iter_max;
    }
    for (size_t i = 0; i < lays.size(); ++i) {
        lays[i].graph = &graphs[i];
        lays[i].params = LayoutSGDParams::from_graph(graphs[i], args.dimensions, args.threads);
        lays[i].params.iter_max = args.layout_iter;
        lays[i].params.progress = args.verbose >= 2;
    }
    HipOptions opt; opt.cfg.n_streams = args.streams; opt.cfg.flags = args.flags | GFS_F_BUNDLE(args.bundle);
    if (args.phased) opt.cfg.flags |= GFS_F_PHASED;                                   // (-p Y only: parse_args)
    const bool measure = args.stress_profile || args.diagnose || args.sort_quality;
    try {
        const double diagnose_ratio = args.diagnose ? args.diagnose_ratio : -1.0;
        const gfs_batch_stats bs = layouts ? sgd_layout_batch(lays, (uint8_t)args.verbose, opt, args.stress_profile, diagnose_ratio)
                                           : sgd_sort_batch(sorts, (uint8_t)args.verbose, opt, measure, args.stress_profile, diagnose_ratio, args.sort_quality);
        for (size_t i = 0; i < files.size(); ++i) {
            const bool batched = layouts ? lays[i].batched : sorts[i].batched;
            const gfs_stats &st = layouts ? lays[i].stats : sorts[i].stats;
            const std::vector<double> &x = layouts ? lays[i].layout.coords : sorts[i].positions;   // empty: nothing was placed
            if (args.verbose >= 1) {
                std::cerr << "[gfasort_hip] " << files[i].in << ": " << graphs[i].node_count() << " nodes, "
                          << (batched ? "in the batch" : st.iterations ? "alone" : "nothing to do") << "\n";
                if (layouts) print_layout_stress(graphs[i], lays[i].layout);
                if (st.iterations) print_run_stats(st);
            }
            if (!measure || x.empty()) continue;
            const std::vector<gfs_pair_error> *resident = !batched ? nullptr : layouts ? &lays[i].profile : &sorts[i].profile;
            const LayoutDiagnosis *diagnosis = !batched || !args.diagnose ? nullptr : layouts ? &lays[i].diagnosis : &sorts[i].diagnosis;
            if (layouts) print_measures(args, graphs[i].flatten(), graphs[i].paths, lays[i].layout.dimensions, x, resident, diagnosis);
            else print_measures(args, sorts[i].before, graphs[i].paths, 0, x, resident, diagnosis, batched && args.sort_quality ? &sorts[i].quality : nullptr);
        }
        if (args.verbose >= 1) print_batch_stats(bs);
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
    for (size_t i = 0; i < lays.size(); ++i) if (!write_layout_file(args, files[i].layout, lays[i].layout)) return 1;
    for (size_t i = 0; i < files.size(); ++i) if (!write_gfa_file(args, files[i].out, graphs[i])) return 1;
    if (warm.joinable()) warm.join();
    std::cerr.flush(); std::cout.flush();
    std::_Exit(0);
}

int main(int argc, char **argv) {
    Args args;
    if (!parse_args(argc, argv, args)) { usage(); return 2; }
    if (validate_pipeline(args.pipeline)) return 1;
    if (!args.batch_list.empty()) return run_batch(args);
    auto t_start = std::chrono::steady_clock::now();
    auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    double t_read = 0, t_parse = 0, t_steps = 0, t_write = 0;
    // bring the HIP context up while the GFA is read and parsed (errors surface later, in the SGD call)
    std::thread warm([] { (void)gfs_warmup(0); });
    Joiner joiner{warm};
    if (args.verbose >= 1) std::cerr << "[gfasort] reading " << args.input << "\n";
    std::string content;
    try { content = read_file(args.input); }
    catch (const std::exception &e) { std::cerr << "Error reading file: " << e.what() << "\n"; return 1; }
    t_read = since(t_start);
    auto t_p0 = std::chrono::steady_clock::now();
    BidirectedGraph graph;
    try { graph = parse_gfa(content); }
    catch (const std::exception &e) { std::cerr << "Error parsing GFA: " << e.what() << "\n"; return 1; }
    t_parse = since(t_p0);
    if (args.verbose >= 1)
        std::cerr << "[gfasort] loaded " << graph.node_count() << " nodes, " << graph.edges.size() << " edges, "
                  << graph.paths.size() << " paths\n";
    if (args.verbose >= 2) std::cerr << "[gfasort] pipeline: " << args.pipeline << "\n";

    YgsParams ygs = YgsParams::from_graph(graph, (uint8_t)args.verbose, args.threads);      // gfasort.rs:222-224
    PathSGDParams sgd_params = ygs.path_sgd;
    sgd_params.iter_max = args.iter_max;
    LayoutSGDParams layout_params = LayoutSGDParams::from_graph(graph, args.dimensions, args.threads);   // :227-229
    layout_params.iter_max = args.layout_iter;
    layout_params.progress = args.verbose >= 2;
    HipOptions opt; opt.cfg.n_streams = args.streams; opt.cfg.flags = args.flags | GFS_F_BUNDLE(args.bundle);

    bool have_layout = false;
    Layout layout;
    const bool measure = args.stress_profile || args.diagnose || args.sort_quality;
    // the warm-up thread is NOT joined here: flattening and parameter scans need no GPU, and the first HIP
    // call of the SGD step simply waits inside the runtime for whatever initialisation is still going on
    auto t_s0 = std::chrono::steady_clock::now();
    try {
        size_t step = 0;
        for (char c : args.pipeline) {
            ++step;
            if (args.verbose >= 1)
                std::cerr << "[gfasort] [" << step << "/" << args.pipeline.size() << "] "
                          << (c == 'Y' ? std::string("SGD") : std::to_string(args.dimensions) + "D layout") << "\n";
            gfs_stats st{};
            if (c == 'Y') {
                HipOptions opt_y = opt;
                if (args.phased) opt_y.cfg.flags |= GFS_F_PHASED;
                // (the profile speaks the dense indices of the graph as it is before the sort reorders it)
                FlatGraph before;
                std::vector<double> x;
                if (measure) before = graph.flatten();
                sgd_sort_only(graph, sgd_params, (uint8_t)args.verbose, opt_y, &st, measure ? &x : nullptr);   // gfasort.rs:250-252
                if (!x.empty()) print_measures(args, before, graph.paths, 0, x);
                if (args.phased && args.verbose >= 2) {
                    uint64_t kb = 0, ke = sgd_params.iter_max + 1;         // reference streams picked: the whole schedule is theirs
                    if (st.bundle == 64) { gfs_sgd_params cp = sgd_params.to_c(); gfs_phase_window(&cp, &kb, &ke); }
                    std::cerr << "[gfasort_hip] phased sampler: reference streams in iterations [" << kb << ", " << ke << ") of 0.."
                              << sgd_params.iter_max << "\n";
                }
            } else {
                layout = path_linear_sgd_layout(graph, layout_params, opt, &st);            // :265-267
                have_layout = true;
                if (args.verbose >= 1) print_layout_stress(graph, layout);
                if (measure && !layout.coords.empty()) print_measures(args, graph.flatten(), graph.paths, layout.dimensions, layout.coords);
            }
            if (args.verbose >= 1 && st.iterations) print_run_stats(st);
        }
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
    t_steps = since(t_s0);
    if (warm.joinable()) warm.join();
    auto t_w0 = std::chrono::steady_clock::now();
    if (have_layout) {
        if (!args.layout_out.empty()) {
            if (!write_layout_file(args, args.layout_out, layout)) return 1;
        } else if (args.verbose >= 1) {
            std::cerr << "[gfasort] warning: layout computed but --layout-out not specified\n";
        }
    }
    if (!write_gfa_file(args, args.output, graph)) return 1;
    t_write = since(t_w0);
    if (args.verbose >= 1) {
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        std::cerr << "[gfasort] done (" << s << " s wall: read " << t_read << ", parse " << t_parse << ", pipeline "
                  << t_steps << ", write " << t_write << ")\n";
    }
    // everything is written and closed: leave without tearing down the graph (millions of small
    // allocations) and the HIP runtime, which costs ~0.1 s and changes nothing on disk
    std::cerr.flush(); std::cout.flush();
    std::_Exit(0);
}
