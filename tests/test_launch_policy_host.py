"""The launch policy (csrc/launch_policy.h) and the host tables (csrc/host_tables.hip) without a device: each compiled with a plain
C++ compiler into a program of its own, under the address and undefined-behaviour sanitizers, and run.  Nothing is loaded into
Python.  Every expectation of the policy cases is worked out by hand from the rule as launch_policy.h states it; the arithmetic
stands beside the case."""
import os
import shutil
import subprocess

from util import ROOT

CSRC = os.path.join(ROOT, "gfasort_amd", "csrc")
SANITIZE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

COMMON = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
"""

POLICY_MAIN = COMMON + r"""
#include "launch_policy.h"
using namespace gfs;

struct Graph {
    std::vector<uint32_t> counts;
    GraphFacts facts;
    Graph(uint64_t n_nodes, std::vector<std::pair<uint32_t, uint32_t>> paths) {      // (how many, steps each)
        for (auto &pc : paths) for (uint32_t k = 0; k < pc.first; ++k) counts.push_back(pc.second);   // exactly n_paths entries
        facts.n_nodes = n_nodes; facts.n_paths = counts.size();
        for (uint32_t c : counts) { facts.n_steps += c; if (c > facts.max_path_steps) facts.max_path_steps = c; if (c > 1) facts.valid_paths = true; }
        facts.path_counts = counts.data();
    }
};
static gfs_sgd_params params(uint64_t min_term_updates) {
    gfs_sgd_params p;
    std::memset(&p, 0, sizeof p);
    p.iter_max = 30; p.iter_with_max_learning_rate = 0; p.min_term_updates = min_term_updates; p.delta = 0.0; p.eps = 0.01;
    p.eta_max = 100.0; p.theta = 0.99; p.space = 1000; p.space_max = 100; p.space_quantization_step = 100; p.cooling_start = 0.5;
    p.nthreads = 1; p.seed = 9399220;
    return p;
}
struct Out { int rc; LaunchShape s; std::string err; };
// both phases; per_cu as the runtime would answer for the fused team kernel
static Out shape(const Graph &g, uint64_t quota, int dims, int per_cu, uint32_t flags = 0, int cu_count = 256, uint64_t n_streams = 0,
                 uint32_t block = 0, uint64_t trace = 0) {
    gfs_sgd_params p = params(quota);
    gfs_launch_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.flags = flags; cfg.n_streams = n_streams; cfg.block_size = block; cfg.trace_per_stream = trace;
    Out o;
    DeviceFacts dev; dev.cu_count = cu_count;
    o.rc = shape_before_residency(g.facts, dev, &p, dims, &cfg, &o.s, &o.err);
    if (o.rc == GFS_OK) shape_after_residency(per_cu, dev, &o.s);
    return o;
}

int main() {
    const Graph small(5000, {{1, 50000}});
    const Graph team(16384, {{16, 4096}});                   // 65 536 steps
    const Graph below(16383, {{16, 4096}});
    const Graph mixed(16384, {{15, 4096}, {32, 128}});      // 61 440 + 4 096 = 65 536 steps
    const Graph shorts(16384, {{1024, 16}});                 // paths of 16 steps: only B = 4 has 4 * B <= 16

    {   // Small graph.  streams: chip 256 * 976 = 249 856; by work ((500 000 + 7) / 8 + 63) / 64 * 64 = 62 528; by nodes
        // 5 000 / 4 = 1 250 -> 19 * 64 = 1 216.  Fewer than 16 384 nodes: reference streams, a run is one trip.
        Out o = shape(small, 500000, 0, 0);
        CHECK(o.rc == GFS_OK && o.s.bundle == 1 && o.s.chain == 1 && o.s.partners == 1 && o.s.n_streams == 1216);
        CHECK(o.s.block == 256 && o.s.quota_total == 500000 && o.s.attempt_factor == 64 && !o.s.team && !o.s.phased);
        // zeta: space 1000 > space_max 100: 100 + 900 / 100 + 1 + 1 = 111 entries; the longest jump min(1000, 49 999) reaches
        // index 100 + 9 + 1 = 110: all 111 staged; LDS 1 * 16 + 111 * 8 = 904 bytes
        CHECK(o.s.zlen_full == 111 && o.s.zlen_staged == 111 && o.s.lds_tables && o.s.lds_bytes == 904 && o.s.atomic_loads);
        // 19 waves -> 1 counter; 500 000 < 2^31: pooled, reference streams fuse
        CHECK(o.s.fused && o.s.pooled && !o.s.fuse_one && !o.s.fuse_one_probe && o.s.one_chunk == TEAM_CHUNK && o.s.fused_resident_blocks == 0);
    }
    {   // Team at the threshold.  First count (reference rule): by work 81 920, by nodes 16 384 / 4 = 4 096 -> 4 096, a multiple of 64.
        // Every path has >= 4 * 64 steps: B = 64, two partners.  K: 655 360 / (64 * 64 * 2) = 80 >= 64 leaders: 64 stays.
        // Team count: chip 256 * 1024; by work 81 920; by nodes 16 384 * 3 / 4 = 12 288.
        Out o = shape(team, 655360, 0, 4);
        CHECK(o.rc == GFS_OK && o.s.bundle == 64 && o.s.partners == 2 && o.s.chain == 64 && o.s.n_streams == 12288 && o.s.team);
        // resident: 4 * 256 = 1 024 workgroups >= the 48 of the launch; 192 waves -> 12 counters, 655 360 / 12 < 2^31
        CHECK(o.s.fused_resident_blocks == 1024 && o.s.fused && o.s.pooled && !o.s.fuse_one && o.s.fuse_one_probe && o.s.one_chunk == 2048);
        CHECK(shape(below, 655360, 0, 4).s.bundle == 1);     // just below the threshold
        CHECK(shape(below, 655360, 0, 4).s.n_streams == 4032);   // 16 383 / 4 = 4 095 -> 63 * 64
    }
    {   // Chain halving: 65 536 / (64 * K * 2) = 8, 16, 32, 64 at K = 64, 32, 16, 8: the first with 64 leaders is K = 8
        Out o = shape(team, 65536, 0, 4);
        CHECK(o.rc == GFS_OK && o.s.bundle == 64 && o.s.chain == 8 && o.s.partners == 2);
        CHECK(o.s.n_streams == 8192);                         // by work: ((65 536 + 7) / 8 + 63) / 64 * 64
        // ... only where the library picked the bundle as well
        CHECK(shape(team, 65536, 0, 4, GFS_F_BUNDLE(64)).s.chain == 64);
        CHECK(shape(team, 65536, 0, 4, GFS_F_CHAIN(32)).s.chain == 32);
        CHECK(shape(team, 655360, 0, 4, GFS_F_ONE_PARTNER).s.partners == 1);
    }
    {   // 95 % rule: 61 440 / 65 536 = 93.75 % of the steps in paths of >= 256 steps, all of them in paths of >= 128
        Out o = shape(mixed, 655360, 0, 4);
        CHECK(o.rc == GFS_OK && o.s.bundle == 32 && o.s.chain == 1 && o.s.partners == 1 && o.s.team);
    }
    {   // Residency bound: chip 8 * 1024 = 8 192 < 12 288; resident 1 * 8 workgroups * 256 = 2 048 lanes
        Out o = shape(team, 655360, 0, 1, 0, 8);
        CHECK(o.rc == GFS_OK && o.s.bundle == 64 && o.s.n_streams == 2048 && o.s.fused_resident_blocks == 8 && o.s.fused && o.s.pooled);
        // an explicit count stays: 16 workgroups > 8 resident: one launch per iteration
        Out e = shape(team, 655360, 0, 1, 0, 8, 4096);
        CHECK(e.rc == GFS_OK && e.s.bundle == 64 && e.s.n_streams == 4096 && !e.s.fused && !e.s.fuse_one_probe);
        // fewer than 64 resident lanes bound nothing (per_cu = 0)
        CHECK(shape(team, 655360, 0, 0, 0, 8).s.n_streams == 8192 && !shape(team, 655360, 0, 0, 0, 8).s.fused);
    }
    {   // Layouts
        CHECK(shape(shorts, 655360, 0, 4).s.bundle == 4);    // the sort takes B = 4 ...
        CHECK(shape(shorts, 655360, 2, 3).s.bundle == 1);    // ... a layout never
        Out e4 = shape(team, 655360, 2, 3, GFS_F_BUNDLE(4));
        CHECK(e4.rc == GFS_E_UNSUPPORTED && e4.err == "bundled layout kernels exist for 1..8 dimensions and bundles of 8..64");
        CHECK(shape(team, 655360, 5, 2).s.bundle == 1);      // 4..8 dimensions: auto keeps reference streams
        Out w = shape(team, 655360, 5, 2, GFS_F_BUNDLE(64));
        // an explicit bundle: K = 16 for layouts, not halved; chip 256 CUs * 256 * 2 waves; by nodes 12 288
        CHECK(w.rc == GFS_OK && w.s.bundle == 64 && w.s.partners == 2 && w.s.chain == 16 && w.s.n_streams == 12288 && w.s.team);
        // fuse_one: 192 waves; 4 * ND_TEAM_CHUNK = 16 384 updates per wave = 3 145 728 per iteration
        Out a = shape(team, 3145728, 2, 3), b = shape(team, 3145727, 2, 3);
        CHECK(a.rc == GFS_OK && a.s.bundle == 64 && a.s.chain == 16 && a.s.n_streams == 12288 && a.s.fused && a.s.pooled && a.s.one_chunk == 4096);
        CHECK(a.s.fused_resident_blocks == 768 && a.s.fuse_one && a.s.fuse_one_probe);
        CHECK(b.rc == GFS_OK && b.s.fused && !b.s.fuse_one && b.s.fuse_one_probe);
        Out blk = shape(team, 655360, 2, 3, 0, 256, 0, 320);
        CHECK(blk.rc == GFS_E_ARG && blk.err == "the layout team kernels are built for workgroups of at most 256 lanes");
        CHECK(shape(team, 655360, 0, 3, 0, 256, 0, 320).rc == GFS_OK);     // the sort's team kernels take it
        CHECK(shape(team, 655360, 0, 3, 0, 256, 0, 96).rc == GFS_E_ARG && shape(team, 655360, 0, 3, 0, 256, 0, 1088).rc == GFS_E_ARG);
    }
    {   // Flags: each of these rules the fused launch out, for team shapes and for reference streams
        CHECK(!shape(team, 655360, 0, 4, GFS_F_NO_FUSE).s.fused && !shape(small, 500000, 0, 0, GFS_F_NO_FUSE).s.fused);
        Out pl = shape(team, 655360, 0, 4, GFS_F_PLAIN_LOADS);
        CHECK(pl.rc == GFS_OK && !pl.s.atomic_loads && !pl.s.fused && !shape(small, 500000, 0, 0, GFS_F_PLAIN_LOADS).s.fused);
        Out tr = shape(team, 655360, 0, 4, 0, 256, 0, 0, 1);
        CHECK(tr.rc == GFS_OK && tr.s.trace && !tr.s.fused && !shape(small, 500000, 0, 0, 0, 256, 0, 0, 1).s.fused);
        CHECK(shape(team, 655360, 0, 4, GFS_F_NO_FUSE).s.fuse_one_probe);   // (the probe knob's answer does not depend on them)
        Out nl = shape(small, 500000, 0, 0, GFS_F_NO_LDS_TABLES);
        CHECK(nl.rc == GFS_OK && !nl.s.lds_tables && nl.s.lds_bytes == 0 && nl.s.fused);
        // free-running: the free kernel for team shapes (fused, not pooled); reference streams keep their pools
        Out fr = shape(team, 655360, 0, 4, GFS_F_DBG_FREE_RUNNING);
        CHECK(fr.rc == GFS_OK && fr.s.fused && !fr.s.pooled && fr.s.fuse_one_probe);
        Out fs = shape(small, 500000, 0, 0, GFS_F_DBG_FREE_RUNNING);
        CHECK(fs.rc == GFS_OK && fs.s.fused && fs.s.pooled);
        // phased: the window around the switch to cooling: first_cooling = floor(0.5 * 30) = 15: [16, 31)
        Out ph = shape(team, 655360, 0, 4, GFS_F_PHASED);
        CHECK(ph.rc == GFS_OK && ph.s.phased && ph.s.bundle == 64 && ph.s.win_begin == 16 && ph.s.win_end == 31 && ph.s.fused && ph.s.pooled);
        Out pf = shape(team, 655360, 0, 4, GFS_F_PHASED | GFS_F_DBG_FREE_RUNNING);
        CHECK(pf.rc == GFS_OK && pf.s.phased && !pf.s.fused);               // the phased sampler has no free-running form
        Out pr = shape(small, 500000, 0, 0, GFS_F_PHASED);                   // reference streams: every iteration is the window's
        CHECK(pr.rc == GFS_OK && !pr.s.phased && pr.s.bundle == 1 && pr.s.win_begin == 0 && pr.s.win_end == 31);
        Out p8 = shape(team, 655360, 0, 4, GFS_F_PHASED | GFS_F_BUNDLE(8));
        CHECK(p8.rc == GFS_E_ARG && p8.err == "GFS_F_PHASED switches between reference streams and bundles of 64: GFS_F_BUNDLE must be 0 or 64");
        Out p2 = shape(team, 655360, 2, 3, GFS_F_PHASED);
        CHECK(p2.rc == GFS_E_ARG && p2.err == "GFS_F_PHASED is a sampler of the 1D sort: layouts have none");
        for (uint32_t k : {3u, 128u, 65u}) {
            Out c = shape(team, 655360, 0, 4, GFS_F_CHAIN(k));
            CHECK(c.rc == GFS_E_ARG && c.err == "GFS_F_CHAIN: the run length in trips must be a power of two <= 64");
        }
        Out b5 = shape(team, 655360, 0, 4, GFS_F_BUNDLE(5));
        CHECK(b5.rc == GFS_E_ARG && b5.err == "bundled sampling needs n_streams % 64 == 0 and a bundle of 4, 8, 16, 32 or 64");
        CHECK(shape(team, 655360, 0, 4, GFS_F_BUNDLE(8), 256, 100).rc == GFS_E_ARG);   // n_streams % 64
        CHECK(shape(team, 655360, 9, 4).rc == GFS_E_UNSUPPORTED && shape(team, 655360, -1, 4).rc == GFS_E_UNSUPPORTED);
        CHECK(shape(team, 655360, 0, 4, 0, 256, 0x80000000ull).rc == GFS_E_ARG);       // n_streams too large
    }
    {   // argument checks and graphs with nothing to do
        gfs_sgd_params p = params(1000);
        LaunchShape s; std::string err; DeviceFacts dev; dev.cu_count = 256;
        CHECK(shape_before_residency(team.facts, dev, nullptr, 0, nullptr, &s, &err) == GFS_E_ARG && err == "params is null");
        p.theta = 1.0;
        CHECK(shape_before_residency(team.facts, dev, &p, 0, nullptr, &s, &err) == GFS_E_ARG && err == "theta must be in [0,1)");
        p = params(1000); p.space_quantization_step = 0;
        CHECK(shape_before_residency(team.facts, dev, &p, 0, nullptr, &s, &err) == GFS_E_ARG && err == "space_quantization_step must be > 0");
        p = params(1000); p.eta_max = 0.0;
        CHECK(shape_before_residency(team.facts, dev, &p, 0, nullptr, &s, &err) == GFS_E_ARG && err == "eta_max must be > 0");
        p = params(1000);
        const Graph single(10, {{10, 1}}), empty(0, {});
        CHECK(shape_before_residency(single.facts, dev, &p, 0, nullptr, &s, &err) == GFS_NOTHING_TO_DO);
        CHECK(shape_before_residency(empty.facts, dev, &p, 0, nullptr, &s, &err) == GFS_NOTHING_TO_DO);
        CHECK(shape_before_residency(team.facts, dev, &p, 0, nullptr, &s, &err) == GFS_OK && s.n_streams == 128);   // by work: 125 -> 128
    }
    {   // Pool limit.  1D: the share of one counter.  64 streams = 1 wave = 1 counter
        CHECK(shape(small, (1ull << 31) - 1, 0, 0, 0, 256, 64).s.pooled && shape(small, (1ull << 31) - 1, 0, 0, 0, 256, 64).s.fused);
        CHECK(!shape(small, 1ull << 31, 0, 0, 0, 256, 64).s.pooled && !shape(small, 1ull << 31, 0, 0, 0, 256, 64).s.fused);
        // 16 384 streams = 256 waves = 16 counters
        Out ok = shape(team, (16ull << 31) - 1, 0, 4, 0, 256, 16384), no = shape(team, 16ull << 31, 0, 4, 0, 256, 16384);
        CHECK(ok.rc == GFS_OK && ok.s.bundle == 64 && ok.s.pooled && ok.s.fused);
        CHECK(no.rc == GFS_OK && !no.s.pooled && !no.s.fused && !no.s.fuse_one_probe);
        CHECK(shape(team, 16ull << 31, 0, 4, GFS_F_DBG_FREE_RUNNING, 256, 16384).s.fused);   // fixed quotas need no pool
        // team layouts draw from ONE counter whatever the number of waves
        Out lo = shape(team, (1ull << 31) - 1, 2, 3), ln = shape(team, 1ull << 31, 2, 3);
        CHECK(lo.rc == GFS_OK && lo.s.bundle == 64 && lo.s.n_streams == 12288 && lo.s.pooled && lo.s.fused);
        CHECK(ln.rc == GFS_OK && !ln.s.pooled && !ln.s.fused);
        CHECK(shape(team, 1ull << 31, 2, 3, GFS_F_BUNDLE(1)).s.pooled);      // reference-stream layouts: a share per counter again
    }
    {   // crowd_kshift: floor(log2(max(per, 1))) + 2 with per = n_steps / (2 * n_streams)
        CHECK(crowd_kshift(0, 1) == 2 && crowd_kshift(2, 1) == 2 && crowd_kshift(4, 1) == 3 && crowd_kshift(6, 1) == 3 && crowd_kshift(8, 1) == 4);
        CHECK(crowd_kshift(7, 1) == 3 && crowd_kshift(3, 0) == 3 && crowd_kshift(~0ull, 0) == 65);
        CHECK(!wide_index(0xFFFFFFFFull, 0) && wide_index(0x100000000ull, 0) && wide_index(0x100000001ull, 0) && wide_index(5, GFS_F_DBG_WIDE_INDEX));
    }
    {   // iter_consts
        gfs_sgd_params p = params(1000);
        std::vector<double> etas(p.iter_max + 1);             // exactly iter_max + 1 entries
        for (size_t k = 0; k < etas.size(); ++k) etas[k] = 100.0 - (double)k;
        LaunchShape s;
        IterConsts a = iter_consts(p, etas, s, 15), b = iter_consts(p, etas, s, 16);       // first_cooling = 15: cooling for k > 15
        CHECK(a.cooling == 0 && b.cooling == 1 && a.eta == 85.0 && b.eta == 84.0 && a._pad == 0 && b._pad == 0);
        CHECK(a.zeta2theta == 1.0 + gfs_fast_precise_pow(0.5, 0.99) && b.zeta2theta == 1.0 + gfs_fast_precise_pow(0.5, 0.001));
        // (1 - 0.99 is 0.01 and a little in binary: alpha = 99.99999999999991, whose integer part is 99)
        CHECK(a.omt_e == 0 && a.omt_fb == 1.0 - 0.99 && a.alpha_e == 99 && a.alpha_fb == 1.0 / (1.0 - 0.99) - 99.0);
        CHECK(b.omt_e == 0 && b.omt_fb == 1.0 - 0.001 && b.alpha_e == 1 && b.alpha_fb == 1.0 / (1.0 - 0.001) - 1.0);
        CHECK(iter_consts(p, etas, s, 0).cooling == 0 && iter_consts(p, etas, s, 30).cooling == 1);
        s.phased = true; s.win_begin = 10; s.win_end = 20;
        CHECK(iter_consts(p, etas, s, 9)._pad == 0 && iter_consts(p, etas, s, 10)._pad == 1 && iter_consts(p, etas, s, 19)._pad == 1 &&
              iter_consts(p, etas, s, 20)._pad == 0);
        CHECK(!in_window(s, 9) && in_window(s, 10) && in_window(s, 19) && !in_window(s, 20));
        s.phased = false;
        CHECK(iter_consts(p, etas, s, 10)._pad == 0 && !in_window(s, 10));
    }
    {   // batch_eligible: the pooled fused reference-stream shape, and each single deviation
        LaunchShape s = shape(small, 500000, 0, 0).s;
        CHECK(batch_eligible(s, false, true, false));
        CHECK(!batch_eligible(s, true, true, false) && !batch_eligible(s, false, false, false) && !batch_eligible(s, false, true, true));
        LaunchShape d = s; d.bundle = 64; CHECK(!batch_eligible(d, false, true, false));
        d = s; d.phased = true; CHECK(!batch_eligible(d, false, true, false));
        d = s; d.fused = false; CHECK(!batch_eligible(d, false, true, false));
        d = s; d.pooled = false; CHECK(!batch_eligible(d, false, true, false));
        CHECK(!batch_eligible(shape(team, 655360, 0, 4).s, false, true, false));
        CHECK(!batch_eligible(shape(small, 500000, 0, 0, GFS_F_NO_FUSE).s, false, true, false));
    }
    CHECK(pool_bytes(3) == 3 * 16 * 16 * 4 && pool_slots(15) == 1 && pool_slots(32) == 2 && pool_slots(4000) == 16 && nd_team_waves(2) == 3 && nd_team_waves(3) == 2);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""

TABLES_MAIN = COMMON + r"""
#include "../../include/gfasort_hip.h"

int main() {
    gfs_sgd_params p;
    std::memset(&p, 0, sizeof p);
    {   // schedule: eta_max * exp(-lambda * |t - t_max|), lambda = ln(eta_max / eps) / (iter_max - 1)
        p.iter_max = 3; p.iter_with_max_learning_rate = 1; p.eps = 0.01; p.eta_max = 4.0;
        std::vector<double> etas(p.iter_max + 1, -1.0);       // exactly iter_max + 1 entries: one written past the end is caught
        CHECK(gfs_sgd_schedule(&p, etas.data()) == GFS_OK);
        const double lambda = std::log(400.0) / 2.0;
        CHECK(etas[1] == 4.0 && etas[0] == etas[2] && std::fabs(etas[2] - 4.0 * std::exp(-lambda)) <= 1e-15 * etas[2]);
        CHECK(std::fabs(etas[3] - 0.01) <= 1e-12);            // 4 * exp(-ln 400)
        CHECK(gfs_sgd_schedule(nullptr, etas.data()) == GFS_E_ARG && gfs_sgd_schedule(&p, nullptr) == GFS_E_ARG);
        CHECK(std::string(gfs_last_error()) == "null argument");
    }
    {   // zeta table: space 5 > space_max 2, step 2: 2 + 3 / 2 + 1 + 1 = 5 entries; [3] is the sum up to i = 2, [4] up to i = 4
        p.space = 5; p.space_max = 2; p.space_quantization_step = 2; p.theta = 0.5;
        CHECK(gfs_zeta_table_len(&p) == 5);
        std::vector<double> z(5, -1.0);
        CHECK(gfs_zeta_table(&p, z.data()) == GFS_OK);
        double sum[6] = {0.0};
        for (int i = 1; i <= 5; ++i) sum[i] = sum[i - 1] + gfs_fast_precise_pow(1.0 / (double)i, 0.5);   // in the reference's order
        CHECK(z[0] == 0.0 && z[1] == sum[1] && z[2] == sum[2] && z[3] == sum[2] && z[4] == sum[4]);
        p.space_quantization_step = 0;
        CHECK(gfs_zeta_table_len(&p) == 0 && gfs_zeta_table(&p, z.data()) == GFS_E_ARG);
        p.space = 2; p.space_quantization_step = 2;           // space <= space_max: space + 1 entries
        CHECK(gfs_zeta_table_len(&p) == 3);
    }
    {   // sort order: ascending, -0.0 == +0.0, ties keep the index order, NaN last
        const std::vector<double> x = {2.0, -0.0, 0.0, 1.0, std::nan(""), 1.0};
        std::vector<uint64_t> order(x.size(), 99);
        CHECK(gfs_sort_order(x.data(), x.size(), order.data()) == GFS_OK);
        CHECK((order == std::vector<uint64_t>{1, 2, 3, 5, 0, 4}));
        CHECK(gfs_sort_order(nullptr, 0, nullptr) == GFS_OK && gfs_sort_order(nullptr, 1, order.data()) == GFS_E_ARG);
    }
    {   // the stress read-out's pairs on a graph of two paths (3 and 5 steps) and on one whose first path has a single step
        const std::vector<uint32_t> node_len = {1, 2, 3};
        const std::vector<uint32_t> step_node = {0, 1, 2, 0, 1, 2, 0, 1};
        const std::vector<uint8_t> rev(8, 0);
        for (const std::vector<uint64_t> &first : {std::vector<uint64_t>{0, 3, 8}, std::vector<uint64_t>{0, 1, 8}}) {
            gfs_graph_view g;
            std::memset(&g, 0, sizeof g);
            g.n_nodes = 3; g.n_steps = 8; g.n_paths = 2;
            g.node_len = node_len.data(); g.step_node = step_node.data(); g.step_is_rev = rev.data(); g.path_first_step = first.data();
            const uint64_t want = 1000;
            std::vector<uint64_t> a(want), b(want), a2(want), b2(want);   // room for exactly sample_count pairs
            uint64_t n = 0, n2 = 0;
            CHECK(gfs_stress_sample_pairs(&g, want, 12345, a.data(), b.data(), &n) == GFS_OK);
            CHECK(n > 0 && n <= want);
            for (uint64_t k = 0; k < n; ++k) {
                CHECK(a[k] < 8 && b[k] < 8 && a[k] != b[k]);
                CHECK((a[k] < first[1]) == (b[k] < first[1]));            // both in the same path
                CHECK(first[1] != 1 || (a[k] >= 1 && b[k] >= 1));         // a path of one step gives no pair
            }
            CHECK(gfs_stress_sample_pairs(&g, want, 12345, a2.data(), b2.data(), &n2) == GFS_OK && n2 == n);
            a.resize(n); b.resize(n); a2.resize(n); b2.resize(n);
            CHECK(a == a2 && b == b2);                                    // the stream is a function of the seed
            CHECK(gfs_stress_sample_pairs(&g, want, 12346, a2.data(), b2.data(), &n2) == GFS_OK);
            CHECK(gfs_stress_sample_pairs(&g, 0, 12345, nullptr, nullptr, &n2) == GFS_OK && n2 == 0);
            CHECK(gfs_stress_sample_pairs(&g, 1, 12345, nullptr, nullptr, &n2) == GFS_E_ARG);
            g.n_steps = 1;
            CHECK(gfs_stress_sample_pairs(&g, want, 12345, a.data(), b.data(), &n2) == GFS_OK && n2 == 0);
        }
    }
    {   // the planner's entry and the error slot
        const uint64_t blocks[3] = {5, 5, 11};
        uint32_t launch_of[3], n = 0;
        CHECK(gfs_batch_plan(blocks, 2, 10, launch_of, &n) == GFS_OK && n == 1);
        CHECK(gfs_batch_plan(blocks, 3, 10, launch_of, &n) == GFS_E_UNSUPPORTED);
        unsigned long long named = 99;
        CHECK(std::sscanf(gfs_last_error(), "batch item %llu", &named) == 1 && named == 2);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def _build_and_run(tmp_path, name, source, extra=()):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / (name + ".cpp")
    src.write_text(source)
    exe = tmp_path / name
    subprocess.check_call([cxx] + SANITIZE + ["-I", CSRC, "-o", str(exe), str(src)] + list(extra))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)


# host_tables.hip as a second translation unit of the program, compiled as plain C++
HOST_TABLES = ["-x", "c++", os.path.join(CSRC, "host_tables.hip")]


def test_policy_under_sanitizers(tmp_path):
    """launch_policy.h in a stand-alone program (host_tables.hip beside it: the policy calls gfs_phase_window, gfs_zeta_table_len
    and gfs_fast_precise_pow through the public header)."""
    _build_and_run(tmp_path, "policy_main", POLICY_MAIN, HOST_TABLES)


def test_host_tables_under_sanitizers(tmp_path):
    """host_tables.hip built with a plain C++ compiler: schedule, zeta table, sort order and the stress read-out's pair stream."""
    _build_and_run(tmp_path, "tables_main", TABLES_MAIN, HOST_TABLES)


def test_host_units_compile_as_plain_cxx(tmp_path):
    """The issue's bar for the two host-only units: plain `g++ -std=c++17 -ffp-contract=off`, warnings as errors."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    tu = tmp_path / "policy_tu.cpp"
    tu.write_text('#include "launch_policy.h"\n')
    for args in ([str(tu)], HOST_TABLES):
        subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-c", "-o", str(tmp_path / "out.o")] + args)
