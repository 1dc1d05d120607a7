"""The record width of the 1D team kernels' trips (csrc/launch_policy.h compact_records, shape_records) without a device: a
stand-alone program under the address and undefined-behaviour sanitizers, in the style of test_launch_policy_host.py.  Every
expectation follows from the rule as sgd_device.h crowd_shift states it: crowd_shift<true> of a pair of records is
max(0, a_i - kshift, a_j - kshift, b_i, b_j), so it is 0 for every pair iff max_a <= kshift and max_b == 0; the high position word of
every record is 0 iff the largest position is below 2^32."""
import os
import shutil
import subprocess

from util import ROOT

CSRC = os.path.join(ROOT, "gfasort_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
HOST_TABLES = ["-x", "c++", os.path.join(CSRC, "host_tables.hip")]

MAIN = r"""
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "launch_policy.h"
using namespace gfs;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// 16 paths of 4096 steps over 16 384 nodes (the auto policy's B = 64 at its threshold), both phases of the policy
static LaunchShape shape(uint32_t flags, int dims = 0, uint64_t trace = 0) {
    std::vector<uint32_t> counts(16, 4096);
    GraphFacts g;
    g.n_nodes = 16384; g.n_paths = 16; g.n_steps = 65536; g.max_path_steps = 4096; g.valid_paths = true; g.path_counts = counts.data();
    gfs_sgd_params p;
    std::memset(&p, 0, sizeof p);
    p.iter_max = 30; p.min_term_updates = 655360; p.eps = 0.01; p.eta_max = 100.0; p.theta = 0.99; p.space = 1000; p.space_max = 100;
    p.space_quantization_step = 100; p.cooling_start = 0.5; p.nthreads = 1; p.seed = 9399220;
    gfs_launch_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.flags = flags; cfg.trace_per_stream = trace;
    DeviceFacts dev; dev.cu_count = 256;
    LaunchShape s; std::string err;
    const int rc = shape_before_residency(g, dev, &p, dims, &cfg, &s, &err);
    CHECK(rc == GFS_OK);
    if (rc == GFS_OK) shape_after_residency(4, dev, &s);
    return s;
}
static RecordFacts facts(uint64_t max_pos, uint32_t max_a, uint32_t max_b, bool have = true) {
    RecordFacts r; r.max_pos = max_pos; r.max_a = max_a; r.max_b = max_b; r.have_trip_rec = have;
    return r;
}

int main() {
    const uint64_t two32 = 1ull << 32;
    LaunchShape team = shape(0);
    CHECK(team.dims == 0 && team.bundle == 64 && !team.trace && !team.phased && !team.compact);   // (nothing is compact before shape_records)

    // the position limit: 2^32 - 1 fits the low word, 2^32 does not
    CHECK(compact_records(team, facts(0, 0, 0), 0));
    CHECK(compact_records(team, facts(two32 - 1, 0, 0), 0));
    CHECK(!compact_records(team, facts(two32, 0, 0), 0));
    CHECK(!compact_records(team, facts((1ull << 55) - 1, 0, 0), 0));
    // the crowding limit at the context's kshift: a - kshift <= 0 for the largest a, and no b at all
    CHECK(compact_records(team, facts(1000, 5, 0), 5));
    CHECK(!compact_records(team, facts(1000, 6, 0), 5));
    CHECK(compact_records(team, facts(1000, 63, 0), 63));
    CHECK(!compact_records(team, facts(1000, 1, 0), 0));
    CHECK(!compact_records(team, facts(1000, 0, 1), 40));             // b counts whatever the onset is
    CHECK(!compact_records(team, facts(1000, 0, 7), 40));
    // no array, no compact records (the allocation failed, or the context belongs to a set)
    CHECK(!compact_records(team, facts(1000, 0, 0, false), 5));
    // the flag overrides an eligible graph, and only that
    LaunchShape full = shape(GFS_F_FULL_RECORDS);
    CHECK(full.bundle == 64 && full.n_streams == team.n_streams && full.fused == team.fused && full.chain == team.chain);
    CHECK(!compact_records(full, facts(1000, 0, 0), 5));
    // the kernels that have a compact build: K1b / K1c at B = 64, no trace, not the phased sampler, not a layout
    CHECK(compact_records(shape(GFS_F_NO_FUSE), facts(1000, 0, 0), 5));
    CHECK(compact_records(shape(GFS_F_DBG_FREE_RUNNING), facts(1000, 0, 0), 5));
    CHECK(compact_records(shape(GFS_F_ONE_PARTNER), facts(1000, 0, 0), 5));
    CHECK(!compact_records(shape(GFS_F_BUNDLE(32)), facts(1000, 0, 0), 5));
    CHECK(!compact_records(shape(GFS_F_BUNDLE(1)), facts(1000, 0, 0), 5));
    CHECK(!compact_records(shape(GFS_F_PHASED), facts(1000, 0, 0), 5));
    CHECK(!compact_records(shape(GFS_F_BUNDLE(64), 0, 4), facts(1000, 0, 0), 5));      // a trace
    CHECK(!compact_records(shape(GFS_F_BUNDLE(64), 2), facts(1000, 0, 0), 5));         // a layout
    // shape_records writes the decision into the shape, at the kshift it is given (crowd_kshift of the final stream count)
    const int32_t k = crowd_kshift(65536, team.n_streams);
    CHECK(team.n_streams == 12288 && k == 3);                             // 16 384 * 3 / 4; 65 536 / 24 576 = 2 -> floor(log2) = 1, + 2
    shape_records(facts(two32 - 1, 3, 0), k, &team); CHECK(team.compact);
    shape_records(facts(two32 - 1, 4, 0), k, &team); CHECK(!team.compact);
    shape_records(facts(two32 - 1, 4, 0), 4, &team); CHECK(team.compact); // (an overridden onset: gfs_ctx_debug_kshift)
    shape_records(facts(two32, 0, 0), k, &team); CHECK(!team.compact);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_record_width_policy_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "record_width_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "record_width_main"
    subprocess.check_call([cxx] + SANITIZE + ["-I", CSRC, "-o", str(exe), str(src)] + HOST_TABLES)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
