"""Batches of layouts and the batched quality read-out (K4c / K6c, K7g), the part that needs no device: the exported symbols, the
argument checks made before any device call, the CLI's argument errors, and the block -> item plan (csrc/batch_readout_plan.h,
what the kernels take every index from) in a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

from util import ROOT
from gfasort_amd import build, hip

E_ARG = -1
NAMES = ("gfs_batch_upload_coords", "gfs_batch_coords", "gfs_batch_pair_errors")


def test_symbols_are_exported_and_listed():
    L = hip.lib()
    hdr = open(os.path.join(ROOT, "include", "gfasort_hip.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in hip.EXPORTS and name + "(" in hdr, name
    for method in ("upload_coords", "coords", "pair_errors"):
        assert callable(getattr(hip.Batch, method))
    from gfasort_amd import sgd
    assert callable(sgd.path_linear_sgd_layout_batch)


def test_null_arguments_are_refused_without_a_device():
    L = hip.lib()
    x = (C.c_double * 4)()
    zs = (C.c_uint64 * 1)(1)
    out = (C.c_uint64 * 6)()
    assert L.gfs_batch_upload_coords(None, x, 4, None) == E_ARG
    assert b"null" in L.gfs_last_error()
    assert L.gfs_batch_coords(None, x, 4, None, None) == E_ARG
    assert L.gfs_batch_pair_errors(None, zs, 1, out, None, None) == E_ARG
    assert b"null" in L.gfs_last_error()


PLAN_MAIN = r"""
#include "batch_readout_plan.h"
#include <cstdio>
#include <vector>
static int failures = 0;
#define EXPECT(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

int main() {
    // ---- K7g: the step counts and, written out by hand, the workgroups each gets alone: ceil(n / 2048) within [1, 2048]
    const std::vector<uint64_t> steps = {0, 1, 2047, 2048, 2049, 500000, 2048ull * 2048ull + 1, 3ull * 2048ull * 2048ull + 5};
    const std::vector<uint64_t> alone = {1, 1, 1, 1, 2, 245, 2048, 2048};
    EXPECT(gfs::Q_BLOCK * gfs::Q_PAIRS_PER_THREAD == 2048 && gfs::Q_MAX_BLOCKS == 2048, "constants");
    for (int rotate = 0; rotate < (int)steps.size(); ++rotate) {          // every item in every place of the row
        std::vector<uint64_t> s, want;
        for (size_t i = 0; i < steps.size(); ++i) { s.push_back(steps[(i + rotate) % steps.size()]); want.push_back(alone[(i + rotate) % steps.size()]); }
        std::vector<uint64_t> first(s.size() + 1);                         // exactly n + 1 entries
        const uint64_t total = gfs::quality_plan(s.data(), s.size(), first.data());
        uint64_t sum = 0;
        for (size_t i = 0; i < s.size(); ++i) {
            EXPECT(gfs::quality_blocks_of(s[i]) == want[i], "quality_blocks_of(%llu) = %u", (unsigned long long)s[i], gfs::quality_blocks_of(s[i]));
            EXPECT(first[i] == sum, "first_block[%zu]", i);
            sum += want[i];
        }
        EXPECT(total == sum && first[s.size()] == sum, "row length %llu, want %llu", (unsigned long long)total, (unsigned long long)sum);
        std::vector<uint32_t> item(total);                                 // exactly one entry per workgroup
        gfs::block_item_table(first.data(), s.size(), item.data());
        uint64_t b = 0;
        for (size_t i = 0; i < s.size(); ++i)
            for (uint64_t local = 0; local < want[i]; ++local, ++b) {
                // the pair (local block, local grid) the item's own launch has: start local * Q_BLOCK + thread, stride grid * Q_BLOCK
                const uint64_t grid = first[item[b] + 1] - first[item[b]];
                EXPECT(item[b] == i && b - first[item[b]] == local && grid == want[i], "workgroup %llu: item %u", (unsigned long long)b, item[b]);
            }
        EXPECT(b == total, "workgroups walked");
    }
    {                                                                      // no item, one item
        uint64_t first1[1] = {7};
        EXPECT(gfs::quality_plan(nullptr, 0, first1) == 0 && first1[0] == 0, "empty row");
        gfs::block_item_table(first1, 0, nullptr);
    }
    // ---- K4c / K6c: words and workgroups of the coordinates
    const std::vector<uint64_t> nodes = {1, 2, 63, 64, 0, 65, 255, 256, 257, 39, 0};
    for (uint32_t D : {2u, 3u}) {
        std::vector<uint64_t> word(nodes.size() + 1), first(nodes.size() + 1);
        const uint64_t blocks = gfs::coord_plan(nodes.data(), nodes.size(), D, word.data(), first.data());
        uint64_t words = 0, sum = 0;
        for (size_t i = 0; i < nodes.size(); ++i) {
            const uint64_t w = nodes[i] * 2 * D, nb = (w + 255) / 256;
            EXPECT(word[i] == words && first[i] == sum, "D=%u item %zu: word offset %llu, first block %llu", D, i, (unsigned long long)word[i], (unsigned long long)first[i]);
            EXPECT(gfs::coord_blocks(w) == nb, "coord_blocks(%llu)", (unsigned long long)w);
            words += w; sum += nb;
        }
        EXPECT(word[nodes.size()] == words && first[nodes.size()] == sum && blocks == sum, "D=%u totals", D);
        std::vector<uint32_t> item(blocks);
        gfs::block_item_table(first.data(), nodes.size(), item.data());
        // every packed word is moved by exactly one (workgroup, thread), and no thread points outside its item
        std::vector<unsigned char> moved(words, 0);
        for (uint64_t b = 0; b < blocks; ++b) {
            const uint32_t i = item[b];
            EXPECT(i < nodes.size() && first[i] <= b && b < first[i + 1], "D=%u workgroup %llu", D, (unsigned long long)b);
            const uint64_t w = nodes[i] * 2 * D;
            EXPECT((b - first[i]) * gfs::COORD_BLOCK < w, "D=%u workgroup %llu has no word", D, (unsigned long long)b);
            for (uint64_t t = (b - first[i]) * gfs::COORD_BLOCK; t < (b - first[i] + 1) * gfs::COORD_BLOCK && t < w; ++t) moved[word[i] + t]++;
        }
        for (uint64_t k = 0; k < words; ++k) EXPECT(moved[k] == 1, "D=%u word %llu moved %d times", D, (unsigned long long)k, moved[k]);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """batch_readout_plan.h in a program of its own, built with -fsanitize=address,undefined: the tables hold exactly as many
    entries as the plan says.  Item step counts 0, 1, 2047, 2048, 2049, 5e5 and two beyond 2048 * 2048, in every place of the row:
    each workgroup's (local block, local grid) is what quality_blocks gives the item alone, the clamp included; and the word
    offsets and workgroups of the coordinates at D = 2 and 3."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)


def test_cli_argument_errors(tmp_path):
    """What --batch refuses before it touches a graph or the device."""
    build.build_host()
    data = os.path.join(ROOT, "tests", "data")
    two = tmp_path / "two.tsv"
    two.write_text(f"{data}/simple.gfa\t{tmp_path}/o.gfa\n")
    three = tmp_path / "three.tsv"
    three.write_text(f"{data}/simple.gfa\t{tmp_path}/o.gfa\t{tmp_path}/o.tsv\n")
    run = lambda *a: subprocess.run([build.CLI] + [str(x) for x in a], capture_output=True, text=True)
    r = run("--batch", two, "-p", "L")
    assert r.returncode != 0 and "line 1" in r.stderr and "in.gfa<TAB>out.gfa<TAB>layout.tsv" in r.stderr, r.stderr
    r = run("--batch", three, "-p", "L", "--layout-out", tmp_path / "l.tsv")
    assert r.returncode != 0 and "--layout-out" in r.stderr and "LIST" in r.stderr, r.stderr
    r = run("--batch", three, "-p", "YL")
    assert r.returncode != 0 and "-p Y or -p L exactly, not -p YL" in r.stderr, r.stderr
    r = run("--batch", three, "-p", "Y")                               # a sort's list has two columns
    assert r.returncode != 0 and "line 1" in r.stderr and "expected in.gfa<TAB>out.gfa\n" in r.stderr, r.stderr
    r = run("--batch", two, "-p", "Y", "--layout-out", tmp_path / "l.tsv")
    assert r.returncode != 0 and "--layout-out belongs to -p L" in r.stderr, r.stderr
    assert not (tmp_path / "o.gfa").exists() and not (tmp_path / "o.tsv").exists()
