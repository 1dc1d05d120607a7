"""The batched diagnosis (K7h / K7i / K7j), the part that needs no device: the exported symbols and the refusals made before any
device call; the plan every kernel index comes from (csrc/batch_readout_plan.h: tile_plan, the tile -> item table, the path and
node prefix sums, the packed layout of the stretched-pair lists) in a program of its own under the address and
undefined-behaviour sanitizers; and the seam facts of the graphs tests/test_gpu_batch_diagnosis.py batches, so that a changed
generator cannot quietly stop reaching them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from util import G, ROOT, load, graph_from_paths
from gfasort_amd import hip, quality

E_ARG = -1
Q_TILE = 512
NAMES = ("gfs_batch_path_offsets", "gfs_batch_path_errors", "gfs_batch_stretched_pairs", "gfs_batch_node_errors",
         "gfs_batch_debug_tile_blocks")


def test_symbols_are_exported_and_listed():
    L = hip.lib()
    hdr = open(os.path.join(ROOT, "include", "gfasort_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in hip.EXPORTS and name + "(" in hdr, name
    for method in ("path_offsets", "path_errors", "stretched_pairs", "node_errors", "debug_tile_blocks"):
        assert callable(getattr(hip.Batch, method))
    assert callable(quality.batch_diagnosis) and callable(quality.diagnosis_rows)


def test_null_arguments_are_refused_without_a_device():
    L = hip.lib()
    out = (C.c_uint64 * 16)()
    totals = (C.c_uint64 * 2)(5, 5)
    assert L.gfs_batch_path_offsets(None, out, 3) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_batch_path_errors(None, 1, 10.0, out, 2, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_batch_stretched_pairs(None, 1, 10.0, out, 1, totals, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_batch_node_errors(None, 1, 10.0, out, 2, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_batch_debug_tile_blocks(None, 1) == E_ARG
    assert not any(out) and list(totals) == [5, 5]


def test_diagnosis_rows_are_device_diagnosis_rows():
    pe = np.zeros(3, dtype=hip.PATH_ERROR_DTYPE)
    pe["steps"], pe["reverse_steps"], pe["pairs"], pe["stretched"] = [5, 2, 0], [1, 0, 0], [4, 1, 0], [2, 0, 0]
    pe["sum_rel_sq"], pe["max_rel_sq"] = [16.0, 9.0, 0.0], [9.0, 9.0, 0.0]
    d = quality.diagnosis_rows(pe, worst=2)
    assert [r["rms_rel"] for r in d["rows"]] == [2.0, 3.0, 0.0] and d["worst"] == [1, 0]
    assert d["rows"][0] == dict(path=0, steps=5, reverse_steps=1, pairs=4, rms_rel=2.0, max_rel=3.0, stretched=2)


PLAN_MAIN = r"""
#include "batch_readout_plan.h"
#include <cstdio>
#include <vector>
static int failures = 0;
#define EXPECT(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)
typedef unsigned long long ull;

int main() {
    EXPECT(gfs::Q_TILE == 512 && gfs::Q_TILE_ROUNDS == 8 && gfs::Q_TILE_MAX_BLOCKS == 16384, "constants");
    // step counts and, written out by hand, the tiles each has alone: ceil(n / 512), none without steps
    const std::vector<uint64_t> steps = {0, 511, 512, 513, 0, 0, 1, 2048, 2049, 35059, 5001, 0};
    const std::vector<uint64_t> alone = {0, 1, 1, 2, 0, 0, 1, 4, 5, 69, 10, 0};
    const std::vector<uint64_t> paths = {0, 3, 1, 0, 2, 0, 1, 1, 1, 12, 1, 0};
    const std::vector<uint64_t> nodes = {0, 7, 0, 9, 1, 0, 1, 2048, 2049, 4955, 2501, 3};
    const size_t n = steps.size();
    for (size_t rotate = 0; rotate < n; ++rotate) {                       // zero-step items first, last and adjacent, in every place
        std::vector<uint64_t> s, want, np, nn;
        for (size_t i = 0; i < n; ++i) {
            const size_t k = (i + rotate) % n;
            s.push_back(steps[k]); want.push_back(alone[k]); np.push_back(paths[k]); nn.push_back(nodes[k]);
        }
        std::vector<uint64_t> first(n + 1);                               // exactly n + 1 entries
        const uint64_t total = gfs::tile_plan(s.data(), n, first.data());
        uint64_t sum = 0;
        for (size_t i = 0; i < n; ++i) {
            EXPECT(gfs::quality_tiles_of(s[i]) == want[i], "quality_tiles_of(%llu) = %llu", (ull)s[i], (ull)gfs::quality_tiles_of(s[i]));
            EXPECT(first[i] == sum, "first_tile[%zu] = %llu, want %llu", i, (ull)first[i], (ull)sum);
            sum += want[i];
        }
        EXPECT(total == sum && first[n] == sum, "flat tiles %llu, want %llu", (ull)total, (ull)sum);
        std::vector<uint32_t> item(total);                                // exactly one entry per flat tile
        gfs::tile_item_table(first.data(), n, item.data());
        // every step of every item lies in exactly one (flat tile, lane slot), inside the item's own table
        uint64_t t = 0;
        for (size_t i = 0; i < n; ++i) {
            uint64_t covered = 0;
            for (uint64_t local = 0; local < want[i]; ++local, ++t) {
                EXPECT(item[t] == i && t - first[item[t]] == local, "flat tile %llu: item %u", (ull)t, item[t]);
                const uint64_t lo = local * gfs::Q_TILE, hi = lo + gfs::Q_TILE < s[i] ? lo + gfs::Q_TILE : s[i];
                EXPECT(lo < s[i] && hi <= s[i] && hi > lo, "flat tile %llu has no step", (ull)t);
                covered += hi - lo;
            }
            EXPECT(covered == s[i], "item %zu: %llu of %llu steps covered", i, (ull)covered, (ull)s[i]);
        }
        EXPECT(t == total, "flat tiles walked");
        // rows per path and per node
        std::vector<uint64_t> fp(n + 1), fn(n + 1);
        const uint64_t tp = gfs::row_offsets(np.data(), n, fp.data()), tn = gfs::row_offsets(nn.data(), n, fn.data());
        uint64_t sp = 0, sn = 0;
        for (size_t i = 0; i < n; ++i) { EXPECT(fp[i] == sp && fn[i] == sn, "row offsets of item %zu", i); sp += np[i]; sn += nn[i]; }
        EXPECT(tp == sp && fp[n] == sp && tn == sn && fn[n] == sn, "row totals");
        // the owner of a union path as the combine finds it: the LAST item whose first path is <= p (items without paths share a boundary)
        for (uint64_t p = 0; p < tp; ++p) {
            size_t lo = 0, hi = n;
            while (hi - lo > 1) { const size_t mid = lo + ((hi - lo) >> 1); if (fp[mid] <= p) lo = mid; else hi = mid; }
            EXPECT(fp[lo] <= p && p < fp[lo + 1], "path %llu: item %zu owns [%llu, %llu)", (ull)p, lo, (ull)fp[lo], (ull)fp[lo + 1]);
        }
        // the packed lists: room for min(cap, n_steps) pairs each, side by side, none overlapping
        for (uint64_t cap : {0ull, 1ull, 7ull, 512ull, 513ull, 40000ull, ~0ull}) {
            std::vector<uint64_t> pair(n + 1);
            const uint64_t room = gfs::stretched_list_plan(s.data(), n, cap, pair.data());
            uint64_t at = 0;
            for (size_t i = 0; i < n; ++i) {
                const uint64_t r = cap < s[i] ? cap : s[i];
                EXPECT(gfs::stretched_room(cap, s[i]) == r && pair[i] == at, "cap %llu item %zu: first pair %llu, want %llu", (ull)cap, i, (ull)pair[i], (ull)at);
                at += r;
            }
            EXPECT(room == at && pair[n] == at, "cap %llu: room %llu, want %llu", (ull)cap, (ull)room, (ull)at);
            if (cap == 0) EXPECT(room == 0, "cap 0 needs no room");
        }
    }
    {                                                                      // no item
        uint64_t first1[1] = {7}, pair1[1] = {7}, row1[1] = {7};
        EXPECT(gfs::tile_plan(nullptr, 0, first1) == 0 && first1[0] == 0, "empty tile plan");
        EXPECT(gfs::stretched_list_plan(nullptr, 0, 9, pair1) == 0 && pair1[0] == 0, "empty list plan");
        EXPECT(gfs::row_offsets(nullptr, 0, row1) == 0 && row1[0] == 0, "empty rows");
        gfs::tile_item_table(first1, 0, nullptr);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """batch_readout_plan.h in a program of its own, built with -fsanitize=address,undefined (it is not loaded into Python): items of
    0, 511, 512, 513, 1, 2048, 2049, 35059 and 5001 steps with step-less items first, last and adjacent, in every rotation; caps 0,
    1, 7, 512, 513, beyond every item and 2^64 - 1.  The tables hold exactly as many entries as the plan says."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "diag_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "diag_plan_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)


# ---- the graphs of tests/test_gpu_batch_diagnosis.py, restated ---------------------------------------------------------------
def _chain(n, seed):
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


def many_short_graph():
    rng = np.random.default_rng(11)
    paths = [rng.integers(0, 500, int(k)).tolist() for k in rng.integers(2, 6, 3000)]
    n = sum(len(p) for p in paths)
    return graph_from_paths(paths, rng.integers(1, 9, 500), rev=(rng.random(n) < 0.3))


def hub_graph():
    rng = np.random.default_rng(12)
    path = [0] * 5001
    path[1::2] = range(1, 2501)
    return graph_from_paths([path], rng.integers(1, 9, 2501))


def _tiles(g):
    return -(-g.n_steps // Q_TILE)


def test_the_batched_graphs_reach_their_seams():
    c2048, c2049, drb1, hub, short = _chain(2048, 1), _chain(2049, 2), load("DRB1-3123.gfa"), hub_graph(), many_short_graph()
    assert [_tiles(g) for g in (c2048, c2049, drb1, hub)] == [4, 5, 69, 10]
    assert c2048.n_steps % Q_TILE == 0                                   # no partial tile
    assert c2049.n_steps - (_tiles(c2049) - 1) * Q_TILE == 1             # a last tile of ONE step
    assert _tiles(load("lil.gfa")) == 1 and _tiles(load("simple.gfa")) == 1
    first = drb1.path_first_step.astype(np.int64)
    assert drb1.n_paths == 12 and np.count_nonzero(first[1:-1] % Q_TILE) >= 10 and np.diff(first).min() > 2 * Q_TILE   # tail partials
    assert hub.n_paths == 1 and hub.n_steps == 5001 and int((hub.step_node[::2] == 0).all())
    first = short.path_first_step.astype(np.int64)
    lens = np.diff(first)
    assert short.n_paths == 3000 and lens.min() == 2 and lens.max() == 5 and _tiles(short) == 21
    assert np.count_nonzero(first[1:-1] % Q_TILE == 0) >= 3              # paths that end exactly where a tile does
    assert np.count_nonzero(first[1:-1] % 64 == 0) >= 30                 # ... and where a round of 64 steps does
    assert np.count_nonzero(first[:-1] // Q_TILE != (first[1:] - 1) // Q_TILE) >= 10     # paths that cross a tile seam
    assert np.bincount(first[:-1] // Q_TILE)[:-1].min() >= 140           # ~150 complete paths per full tile
