"""The batched sort quality (K7k, batch_sort_quality_kernels.hip), the part that needs no device: the exported symbols and the
refusals made before any device call; the grouping of a batch's items by padded segment length (csrc/batch_readout_plan.h
segment_launch_order, which gfs_batch_results and gfs_batch_sort_quality both launch by) in a program of its own under the address
and undefined-behaviour sanitizers; the block scan and the scatter by rank restated serially in the kernel's chunking; and the seam
facts of the graphs tests/test_gpu_batch_sort_quality.py batches, so that a changed generator cannot quietly stop reaching them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import ROOT
from gfasort_amd import hip, quality
from quality_restatement import quality_blocks_of
import batch_sort_quality_cases as K

E_ARG = -1
NAMES = ("gfs_batch_sort_quality", "gfs_sort_quality_of")


def test_symbols_are_exported_and_listed():
    L = hip.lib()
    hdr = open(os.path.join(ROOT, "include", "gfasort_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in hip.EXPORTS and name + "(" in hdr, name
    assert callable(hip.Batch.sort_quality) and callable(hip.sort_quality) and callable(quality.sort_quality_figures)


def test_null_arguments_are_refused_without_a_device():
    L = hip.lib()
    out = (C.c_uint64 * 8)(*([7] * 8))
    x = (C.c_double * 2)(1.0, 2.0)
    v = hip.GraphView()
    v.n_nodes = 2
    assert L.gfs_batch_sort_quality(None, out, 2, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_sort_quality_of(None, x, out) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_sort_quality_of(C.byref(v), x, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_sort_quality_of(C.byref(v), None, out) == E_ARG and b"null" in L.gfs_last_error()
    assert list(out) == [7] * 8


def test_the_figures_are_one_derivation():
    q = quality.sort_quality_figures(4, 10, 20, 36.0)
    assert q == dict(steps=4, abs_err_sum=10, genomic_sum=20, sq_err_sum=36.0, mse=9.0, rmse=3.0, mae=2.5, relative_error=0.5)
    z = quality.sort_quality_figures(0, 0, 0, 0.0)
    assert z["rmse"] == 0.0 and z["mae"] == 0.0 and z["relative_error"] == 0.0 and z["steps"] == 0


PLAN_MAIN = r"""
#include "batch_readout_plan.h"
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>
static int failures = 0;
#define EXPECT(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)
typedef unsigned long long ull;

int main() {
    const std::vector<uint64_t> nodes = {0, 1, 63, 64, 65, 128, 129, 4955, 8192, 8193};
    // written out by hand: the padded length of each within the default cap
    const std::vector<uint64_t> padded = {64, 64, 64, 64, 128, 128, 256, 8192, 8192, 0};
    const size_t n = nodes.size();
    for (uint64_t cap : {8192ull, 128ull, 64ull}) {
        for (size_t rotate = 0; rotate < n; ++rotate) {
            std::vector<uint64_t> nn, pp;
            for (size_t i = 0; i < n; ++i) { nn.push_back(nodes[(i + rotate) % n]); pp.push_back(padded[(i + rotate) % n]); }
            std::vector<uint64_t> order(n, ~0ull);                        // exactly n entries
            const uint64_t within = gfs::segment_launch_order(nn.data(), n, cap, order.data());
            // what the call replaced: a stable sort by the padded length, those above the cap last
            std::vector<uint64_t> want(n);
            std::iota(want.begin(), want.end(), 0ull);
            auto key = [&](uint64_t i) { return nn[i] <= cap ? (uint64_t)gfs::segment_padded((uint32_t)nn[i]) : ~0ull; };
            std::stable_sort(want.begin(), want.end(), [&](uint64_t a, uint64_t b) { return key(a) < key(b); });
            EXPECT(order == want, "cap %llu rotation %zu: not the stable sort", (ull)cap, rotate);
            std::vector<int> seen(n, 0);
            uint64_t expect_within = 0;
            for (size_t i = 0; i < n; ++i) expect_within += nn[i] <= cap;
            EXPECT(within == expect_within, "cap %llu rotation %zu: %llu within, want %llu", (ull)cap, rotate, (ull)within, (ull)expect_within);
            for (size_t r = 0; r < n; ++r) {
                EXPECT(order[r] < n, "row %zu names no item", r);
                if (order[r] >= n) continue;
                seen[order[r]]++;
                const uint64_t g = gfs::segment_group_of(nn[order[r]], cap);
                if (r < within) {
                    EXPECT(nn[order[r]] <= cap && g != gfs::SEGMENT_ABOVE_CAP && g >= 64 && (g & (g - 1)) == 0 && g >= nn[order[r]] && g <= gfs::SEGMENT_SORT_CAP,
                           "row %zu: padded length %llu of %llu nodes", r, (ull)g, (ull)nn[order[r]]);
                    if (cap == 8192) EXPECT(g == pp[order[r]], "row %zu: padded %llu, want %llu", r, (ull)g, (ull)pp[order[r]]);
                } else {
                    EXPECT(nn[order[r]] > cap && g == gfs::SEGMENT_ABOVE_CAP, "row %zu: within the cap, behind the launches", r);
                }
                if (r > 0) {
                    const uint64_t before = gfs::segment_group_of(nn[order[r - 1]], cap);
                    EXPECT(before <= g, "row %zu: padded lengths descend", r);                       // ascending; above the cap last
                    if (before == g) EXPECT(order[r - 1] < order[r], "row %zu: item order not kept inside a group", r);
                }
            }
            for (size_t i = 0; i < n; ++i) EXPECT(seen[i] == 1, "item %zu appears %d times", i, seen[i]);
            // the launches: consecutive rows of one padded length, all of them, none twice
            uint64_t first = 0, launches = 0, last_P = 0;
            while (first < within) {
                const uint64_t end = gfs::segment_launch_end(nn.data(), order.data(), first, within, cap);
                EXPECT(end > first && end <= within, "launch at row %llu ends at %llu", (ull)first, (ull)end);
                if (end <= first) break;
                const uint64_t P = gfs::segment_group_of(nn[order[first]], cap);
                EXPECT(P > last_P, "launch at row %llu repeats a padded length", (ull)first);
                for (uint64_t r = first; r < end; ++r) EXPECT(gfs::segment_group_of(nn[order[r]], cap) == P, "row %llu in the wrong launch", (ull)r);
                last_P = P; first = end; ++launches;
            }
            EXPECT(launches <= 8, "%llu launches", (ull)launches);
            if (cap == 8192) EXPECT(launches == 4, "cap 8192: %llu launches, want 64, 128, 256, 8192", (ull)launches);
            if (cap == 64) EXPECT(launches == 1 && within == 4, "cap 64: one launch of four items");
        }
    }
    {                                                                      // no item
        EXPECT(gfs::segment_launch_order(nullptr, 0, 8192, nullptr) == 0, "empty order");
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """segment_launch_order and segment_launch_end in a program of its own, built with -fsanitize=address,undefined (it is not loaded
    into Python): node counts 0, 1, 63, 64, 65, 128, 129, 4955, 8192, 8193 in every rotation, caps 8192, 128 and 64.  Groups in
    ascending padded length, item order kept inside a group, items above the cap last and in order, every item exactly once."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "segment_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "segment_plan_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)


def test_the_restated_launch_order_is_the_plans_on_the_same_inputs():
    nodes = [0, 1, 63, 64, 65, 128, 129, 4955, 8192, 8193]
    assert K.launch_order(nodes, 8192) == ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], 9)
    assert K.launch_order(nodes, 64) == ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], 4)
    assert K.launch_order(nodes[::-1], 128) == ([9, 8, 7, 6, 5, 4, 3, 2, 1, 0][:0] + [6, 7, 8, 9, 4, 5, 0, 1, 2, 3], 6)


@pytest.mark.parametrize("block", [64, 128, 1024])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 8192])
def test_the_block_scan_and_the_scatter_by_rank_are_a_prefix_sum(block, n):
    """The chunked scan of one workgroup — waves of 64, totals in wave order, a carry from chunk to chunk — equals np.cumsum in
    u64 over lengths up to 2^32 - 1, and every node's slot receives the prefix of its rank."""
    rng = np.random.default_rng(1000 * block + n)
    node_len = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    node_len[rng.integers(0, n, max(n // 8, 1))] = 2 ** 32 - 1
    index = rng.permutation(n)                                           # rank -> dense index
    perm = rng.permutation(n)                                            # dense index -> slot
    spos, total = K.block_scan_scatter(node_len[index], index, perm, block)
    prefix = np.concatenate([[0], np.cumsum(node_len[index], dtype=np.uint64)[:-1]]).astype(np.uint64)
    want = np.zeros(n, dtype=np.uint64)
    want[perm[index]] = prefix
    assert spos.dtype == np.uint64 and np.array_equal(spos, want)
    assert total == int(node_len.sum(dtype=np.uint64)) and (n < 3 or total > 2 ** 32)


def test_the_batched_graphs_reach_their_seams():
    gs = dict(zip(K.NAMES, K.graphs()))
    padded = {k: K.segment_padded(g.n_nodes) for k, g in gs.items() if g.n_nodes <= K.SEGMENT_SORT_CAP}
    assert padded == dict(simple=64, lil=64, DRB1=8192, chain64=64, chain65=128, chain1025=2048, chain2049=4096, one_node=64,
                          one_step=64, absent_node=64)
    assert gs["DRB1"].n_nodes == 4955 and gs["DRB1"].n_steps == 35059 and quality_blocks_of(35059) == 18
    assert 12 * padded["DRB1"] == 96 * 1024                              # the launch that needs its dynamic LDS limit raised
    assert K.segment_block(64) == 64 and K.segment_block(128) == 64      # one wave: P = 64 has no LDS stage, P = 128 the first
    assert gs["chain64"].n_nodes == 64 and gs["chain65"].n_nodes == 65
    assert gs["chain1025"].n_nodes == 1025 and K.segment_block(padded["chain1025"]) == 1024     # 16 waves, two chunks of the scan
    assert gs["chain2049"].n_steps == 2049 and quality_blocks_of(2049) == 2 and quality_blocks_of(2048) == 1
    assert gs["one_node"].n_nodes == 1 and gs["one_node"].n_steps == 3
    assert gs["one_step"].n_paths == 1 and gs["one_step"].n_steps == 1
    assert int((gs["absent_node"].step_node == 0xFFFFFFFF).sum()) == 1
    m = gs["medium"]
    assert [k for k, g in gs.items() if g.n_steps > 256 * 2048] == ["medium"] and m.n_steps == 524288 + 1000
    assert quality_blocks_of(m.n_steps) == 257 and m.n_nodes > K.SEGMENT_SORT_CAP                # a second tile of partials; K6's path
    # with the cap lowered to 128 and 64 items move from the LDS path to K6's
    for cap, within in ((8192, 10), (128, 7), (64, 6)):
        assert K.launch_order([g.n_nodes for g in gs.values()], cap)[1] == within
    first_block = np.concatenate([[0], np.cumsum([quality_blocks_of(g.n_steps) for g in gs.values()])])
    assert first_block[-1] == 1 + 1 + 18 + 1 + 1 + 1 + 2 + 1 + 1 + 1 + 257 and first_block[10] > 0        # medium's partials do not start the row
