"""The byte maps of the read-outs (csrc/readout_region.h gfs::Region), the part that needs no device.  Every read-out works in one
allocation, [tables that go up | results that come back | scratch that never leaves]; seven batch entries (capi_batch.hip) and six
context entries (capi.hip) build their map with Region.  Here each map's formula stands written out as plain arithmetic, as the
entries had it before Region: the offsets, the size of the pinned staging, the size of the device buffer.  A program of its own,
built from readout_region.h and batch_readout_plan.h under the address and undefined-behaviour sanitizers (it is not loaded into
Python), builds the same maps from the same counts, and every figure must be equal.

One figure is not what the formulas before Region gave: gfs_batch_path_errors, gfs_batch_stretched_pairs and gfs_batch_node_errors
sent their two tables up to the start of the next part, which is the end of the second table rounded up to 8 bytes; uploaded() is
the end of the table itself, as gfs_batch_pair_errors and gfs_batch_sort_quality always had it.  The difference is padding that
no kernel reads, at most 4 bytes, and the test holds it to that."""
import os
import shutil
import subprocess

import pytest

from util import ROOT

# sizeof of the records a map holds: static_asserted next to the structs in csrc/sgd_host.h (which includes the HIP runtime and so
# cannot be compiled here) and, for the ABI's three, in csrc/capi_ctx.h
READOUT_ITEM, COORD_ITEM, QUALITY_ITEM, DIAG_ITEM, SORT_QUALITY_ITEM = 40, 40, 40, 96, 32
PATH_ERROR, STRETCHED_PAIR, NODE_ERROR = 64, 40, 24
SIZES = (READOUT_ITEM, COORD_ITEM, QUALITY_ITEM, DIAG_ITEM, SORT_QUALITY_ITEM, PATH_ERROR, STRETCHED_PAIR, NODE_ERROR)
Q_BLOCK_STEPS, Q_MAX_BLOCKS, Q_TILE, COORD_BLOCK = 256 * 8, 2048, 512, 256


def w8(b):
    return (b + 7) // 8 * 8


def ceil_div(a, b):
    return -(-a // b)


def blocks_of(steps):
    return min(max(ceil_div(steps, Q_BLOCK_STEPS), 1), Q_MAX_BLOCKS)


# ---- the formulas, as the entries wrote them by hand: name -> ([(offset, bytes) per part], uploaded, staged, bytes) -------------
def maps_of(case):
    """case: dict(items=[(steps, nodes, paths)], dims, n_z, cap, tmp_bytes, n_list).  An entry that returns before it builds its map
    (no coordinate, no path, no tile, no node: nothing to do) has no formula for that case."""
    items, D, n_z, cap, tmp_bytes, n_list = (case[k] for k in ("items", "dims", "n_z", "cap", "tmp_bytes", "n_list"))
    n = len(items)
    rb = sum(blocks_of(s) for s, _, _ in items)                          # quality_plan
    tiles = sum(ceil_div(s, Q_TILE) for s, _, _ in items)                # tile_plan
    nodes = sum(k for _, k, _ in items)
    paths = sum(p for _, _, p in items)
    pairs = sum(min(cap, s) for s, _, _ in items)                        # stretched_list_plan
    words = sum(k * 2 * D for _, k, _ in items)                          # coord_plan
    cblocks = sum(ceil_div(k * 2 * D, COORD_BLOCK) for _, k, _ in items)
    out = {}

    # gfs_batch_results: the pinned staging alone [positions | order] (the device side is two buffers of its own)
    out["batch_results"] = ([(0, nodes * 8), (nodes * 8, nodes * 4)], 0, nodes * 12, nodes * 12)

    # batch_coords_move: [packed coordinates | CoordItem table | block table]; up, the whole of it goes
    tables_at = words * 8
    blocks_at = tables_at + n * COORD_ITEM
    total = blocks_at + cblocks * 4
    if words:
        out["batch_coords"] = ([(0, words * 8), (tables_at, n * COORD_ITEM), (blocks_at, cblocks * 4)], total, total, total)

    # gfs_batch_pair_errors: [zs | QualityItem table | block table (whole words) | out words | partials]
    items_at = n_z * 8
    blocks_at = items_at + n * QUALITY_ITEM
    out_at = blocks_at + (rb * 4 + 7) // 8 * 8
    out_bytes = n * n_z * 5 * 8
    partials_at = out_at + out_bytes
    total = partials_at + 5 * n_z * rb * 8
    out["batch_pair_errors"] = ([(0, n_z * 8), (items_at, n * QUALITY_ITEM), (blocks_at, rb * 4), (out_at, out_bytes),
                                 (partials_at, 5 * n_z * rb * 8)], blocks_at + rb * 4, out_at + out_bytes, total)

    # gfs_batch_sort_quality: [ReadoutItem rows | SortQualityItem table | block table (whole words) | out words | totals by row |
    # sorted positions | partials]
    items_at = n * READOUT_ITEM
    blocks_at = items_at + n * SORT_QUALITY_ITEM
    out_at = blocks_at + w8(rb * 4)
    totals_at = out_at + n * 5 * 8
    spos_at = totals_at + n * 8
    partials_at = spos_at + nodes * 8
    total = partials_at + 5 * rb * 8
    out["batch_sort_quality"] = ([(0, n * READOUT_ITEM), (items_at, n * SORT_QUALITY_ITEM), (blocks_at, rb * 4), (out_at, n * 40),
                                  (totals_at, n * 8), (spos_at, nodes * 8), (partials_at, 5 * rb * 8)], blocks_at + rb * 4, spos_at, total)

    # gfs_batch_path_errors: [DiagItem table | tile table (whole words) | out | head partials | tail partials]
    tiles_at = n * DIAG_ITEM
    out_at = tiles_at + w8(tiles * 4)
    out_bytes = paths * PATH_ERROR
    head_at = out_at + out_bytes
    tail_at = head_at + 5 * tiles * 8
    total = tail_at + 5 * tiles * 8
    if paths:
        out["batch_path_errors"] = ([(0, n * DIAG_ITEM), (tiles_at, tiles * 4), (out_at, out_bytes), (head_at, 5 * tiles * 8),
                                     (tail_at, 5 * tiles * 8)], tiles_at + tiles * 4, out_at + out_bytes, total)
    assert w8(tiles_at + tiles * 4) == out_at                            # (what went up before: to out_at, padding included)

    # gfs_batch_stretched_pairs: [DiagItem table | tile table (whole words) | tile counts | offsets | list | the scan's storage],
    # the storage at least 8 bytes
    counts_at = tiles_at + w8(tiles * 4)
    offsets_at = counts_at + (tiles + 1) * 8
    list_at = offsets_at + (tiles + 1) * 8
    tmp_at = list_at + pairs * STRETCHED_PAIR
    tmp = tmp_bytes if tmp_bytes else 8
    if tiles:
        out["batch_stretched_pairs"] = ([(0, n * DIAG_ITEM), (tiles_at, tiles * 4), (counts_at, (tiles + 1) * 8), (offsets_at, (tiles + 1) * 8),
                                         (list_at, pairs * STRETCHED_PAIR), (tmp_at, tmp)], tiles_at + tiles * 4, tmp_at, tmp_at + tmp)
    assert w8(tiles_at + tiles * 4) == counts_at

    # gfs_batch_node_errors: [DiagItem table | block table (whole words) | out | per slot: pairs, stretched, max]
    blocks_at = n * DIAG_ITEM
    out_at = blocks_at + w8(rb * 4)
    out_bytes = nodes * NODE_ERROR
    slots_at = out_at + out_bytes
    if nodes:
        out["batch_node_errors"] = ([(0, n * DIAG_ITEM), (blocks_at, rb * 4), (out_at, out_bytes), (slots_at, out_bytes)],
                                    blocks_at + rb * 4, out_at + out_bytes, slots_at + out_bytes)
    assert w8(blocks_at + rb * 4) == out_at

    # the context entries, on item 0: maps in 8-byte words, nothing staged, copies of their own
    steps, k, p = items[0]
    blocks, tiles = blocks_of(steps), ceil_div(steps, Q_TILE)
    room = min(cap, steps)

    def words_map(*parts):                                               # parts in words, side by side
        at, rows = 0, []
        for w in parts:
            rows.append((8 * at, 8 * w))
            at += w
        return rows, 0, 0, 8 * at
    out["ctx_pair_errors"] = words_map(n_z, 5 * n_z, 5 * n_z * blocks)             # 8 * (n_z + 5 * n_z + 5 * n_z * blocks)
    out["ctx_stress_of_pairs"] = words_map(n_list, n_list, n_list)                 # 8 * 3 * n
    out["ctx_sort_quality"] = words_map(k + 1, k, 5 * blocks, 5)                   # 8 * ((n + 1) + n + 5 * blocks + 5)
    if p:
        out["ctx_path_errors"] = words_map(8 * p, 5 * tiles, 5 * tiles)            # 8 * (8 * n_paths + 10 * tiles)
    out["ctx_stretched_pairs"] = words_map(tiles + 1, tiles + 1, 5 * room)         # 8 * (2 * (tiles + 1) + 5 * room)
    if k:
        out["ctx_node_errors"] = words_map(3 * k, 3 * k)                           # 8 * 6 * n_nodes
    return out


def case(items, dims=2, n_z=1, cap=4, tmp_bytes=767, n_list=3):
    return dict(items=list(items), dims=dims, n_z=n_z, cap=cap, tmp_bytes=tmp_bytes, n_list=n_list)


# (steps, nodes, paths) per item
CASES = [
    case([(5, 3, 1)]),                                                   # one item, one step distance, one workgroup: tables of 1 entry
    case([(1025, 7, 2)], n_z=3),                                         # a tile table of 3 entries (12 bytes -> 16), a block table of 1
    case([(2 * 2048 + 1, 9, 1)], dims=1),                                # a block table of 3 entries from one item
    case([(5, 3, 1), (9, 4, 2), (600, 70, 3)], dims=3, n_z=2),           # three items: block table of 3, tile table of 4 (whole words)
    case([(5, 3, 1), (0, 0, 0), (600, 65, 3)], cap=1),                   # a batch of 3 items with one empty item
    case([(5, 3, 1)], cap=0),                                            # no pair listed
    case([(5, 3, 1), (9, 4, 2)], tmp_bytes=0),                           # the scan asks for no storage: the floor of 8 bytes
    case([(5, 3, 1)], tmp_bytes=3),                                      # ... and for an odd amount
    case([(0, 0, 0)]),                                                   # zero nodes in total
    case([(0, 0, 0), (0, 0, 0), (0, 0, 0)], cap=0, tmp_bytes=0),
    case([(3, 2, 2), (0, 1, 0), (0, 0, 1)], cap=10 ** 6),                # paths without steps, a cap above every total
    case([(40000, 129, 12), (513, 64, 1)], dims=2, n_z=7, cap=513, tmp_bytes=1024, n_list=1),
]

MAIN = r"""
#include "readout_region.h"
#include "batch_readout_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef unsigned long long ull;
using gfs::Region;

static std::vector<std::pair<uint64_t, uint64_t>> parts;
static uint64_t part(Region &r, uint64_t bytes) { const uint64_t at = r.add(bytes); parts.push_back({at, bytes}); return at; }
static void emit(int c, const char *name, const Region &r) {
    std::printf("%d %s", c, name);
    for (auto &p : parts) std::printf(" %llu:%llu", (ull)p.first, (ull)p.second);
    std::printf(" | %llu %llu %llu\n", (ull)r.uploaded(), (ull)r.staged(), (ull)r.bytes());
    parts.clear();
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    ull sz[8], n_cases = 0;
    for (ull &s : sz) if (std::fscanf(f, "%llu", &s) != 1) return 2;
    const uint64_t READOUT_ITEM = sz[0], COORD_ITEM = sz[1], QUALITY_ITEM = sz[2], DIAG_ITEM = sz[3], SORT_QUALITY_ITEM = sz[4];
    const uint64_t PATH_ERROR = sz[5], STRETCHED_PAIR = sz[6], NODE_ERROR = sz[7];
    if (std::fscanf(f, "%llu", &n_cases) != 1) return 2;
    for (int c = 0; c < (int)n_cases; ++c) {
        ull D, n_z, cap, tmp_bytes, n_list, n;
        if (std::fscanf(f, "%llu %llu %llu %llu %llu %llu", &D, &n_z, &cap, &tmp_bytes, &n_list, &n) != 6) return 2;
        std::vector<uint64_t> steps(n), nodes(n), paths(n), first(n + 1), word_offset(n + 1);
        for (ull i = 0; i < n; ++i) {
            ull s, k, p;
            if (std::fscanf(f, "%llu %llu %llu", &s, &k, &p) != 3) return 2;
            steps[i] = s; nodes[i] = k; paths[i] = p;
        }
        const uint64_t row_blocks = gfs::quality_plan(steps.data(), n, first.data());
        const uint64_t tiles = gfs::tile_plan(steps.data(), n, first.data());
        const uint64_t total_nodes = gfs::row_offsets(nodes.data(), n, first.data());
        const uint64_t total_paths = gfs::row_offsets(paths.data(), n, first.data());
        const uint64_t pairs = gfs::stretched_list_plan(steps.data(), n, cap, first.data());
        const uint64_t coord_blocks = gfs::coord_plan(nodes.data(), n, (uint32_t)D, word_offset.data(), first.data());
        const uint64_t words = word_offset[n];
        {   // gfs_batch_results
            Region r;
            part(r, total_nodes * 8); part(r, total_nodes * 4);
            r.end_staging();
            emit(c, "batch_results", r);
        }
        {   // batch_coords_move
            Region r;
            part(r, words * 8); part(r, n * COORD_ITEM); part(r, coord_blocks * 4);
            r.end_upload(); r.end_staging();
            emit(c, "batch_coords", r);
        }
        {   // gfs_batch_pair_errors
            Region r;
            part(r, n_z * 8); part(r, n * QUALITY_ITEM); part(r, row_blocks * 4);
            r.end_upload();
            part(r, n * n_z * 5 * 8);
            r.end_staging();
            part(r, 5 * n_z * row_blocks * 8);
            emit(c, "batch_pair_errors", r);
        }
        {   // gfs_batch_sort_quality
            Region r;
            part(r, n * READOUT_ITEM); part(r, n * SORT_QUALITY_ITEM); part(r, row_blocks * 4);
            r.end_upload();
            part(r, n * 5 * 8); part(r, n * 8);
            r.end_staging();
            part(r, total_nodes * 8); part(r, 5 * row_blocks * 8);
            emit(c, "batch_sort_quality", r);
        }
        {   // gfs_batch_path_errors
            Region r;
            part(r, n * DIAG_ITEM); part(r, tiles * 4);
            r.end_upload();
            part(r, total_paths * PATH_ERROR);
            r.end_staging();
            part(r, 5 * tiles * 8); part(r, 5 * tiles * 8);
            emit(c, "batch_path_errors", r);
        }
        {   // gfs_batch_stretched_pairs
            Region r;
            part(r, n * DIAG_ITEM); part(r, tiles * 4);
            r.end_upload();
            part(r, (tiles + 1) * 8); part(r, (tiles + 1) * 8); part(r, pairs * STRETCHED_PAIR);
            r.end_staging();
            part(r, tmp_bytes ? tmp_bytes : 8);
            emit(c, "batch_stretched_pairs", r);
        }
        {   // gfs_batch_node_errors
            Region r;
            part(r, n * DIAG_ITEM); part(r, row_blocks * 4);
            r.end_upload();
            part(r, total_nodes * NODE_ERROR);
            r.end_staging();
            part(r, total_nodes * NODE_ERROR);
            emit(c, "batch_node_errors", r);
        }
        // the context entries, on item 0
        const uint64_t s0 = steps[0], k0 = nodes[0], p0 = paths[0];
        const uint64_t blocks = gfs::quality_blocks_of(s0), t0 = gfs::quality_tiles_of(s0), room = gfs::stretched_room(cap, s0);
        { Region r; part(r, n_z * 8); part(r, 5 * n_z * 8); part(r, 5 * n_z * blocks * 8); emit(c, "ctx_pair_errors", r); }
        { Region r; part(r, n_list * 8); part(r, n_list * 8); part(r, n_list * 8); emit(c, "ctx_stress_of_pairs", r); }
        { Region r; part(r, (k0 + 1) * 8); part(r, k0 * 8); part(r, 5 * blocks * 8); part(r, 5 * 8); emit(c, "ctx_sort_quality", r); }
        { Region r; part(r, p0 * PATH_ERROR); part(r, 5 * t0 * 8); part(r, 5 * t0 * 8); emit(c, "ctx_path_errors", r); }
        { Region r; part(r, (t0 + 1) * 8); part(r, (t0 + 1) * 8); part(r, room * STRETCHED_PAIR); emit(c, "ctx_stretched_pairs", r); }
        { Region r; part(r, k0 * NODE_ERROR); part(r, k0 * NODE_ERROR); emit(c, "ctx_node_errors", r); }
    }
    std::fclose(f);
    {   // at<T>: the part of an allocation, and a part of no bytes between two others
        alignas(8) unsigned char base[64] = {};
        Region r;
        const uint64_t a = r.add(4), z = r.add(0), b = r.add(12);
        *Region::at<uint32_t>(base, a) = 7u;
        *Region::at<uint64_t>(base, b) = 9ull;
        const bool ok = a == 0 && z == 8 && b == 8 && r.bytes() == 20 && base[0] == 7 && base[8] == 9 && Region().add(0) == 0 && Region().bytes() == 0;
        std::printf("accessor %s\n", ok ? "ok" : "BAD");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def built_maps(tmp_path_factory):
    """The program's maps of every case: {(case index, name): ([(offset, bytes)], uploaded, staged, bytes)}, from one run."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    tmp = tmp_path_factory.mktemp("readout_region")
    src, exe, inp = tmp / "region_main.cpp", tmp / "region_main", tmp / "cases.txt"
    src.write_text(MAIN)
    lines = [" ".join(map(str, SIZES)), str(len(CASES))]
    for c in CASES:
        lines.append("%d %d %d %d %d %d" % (c["dims"], c["n_z"], c["cap"], c["tmp_bytes"], c["n_list"], len(c["items"])))
        lines += ["%d %d %d" % it for it in c["items"]]
    inp.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and "accessor ok" in r.stdout, (r.stdout, r.stderr)
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("accessor"):
            continue
        head, marks = line.split(" | ")
        c, name, *parts = head.split()
        got[int(c), name] = ([tuple(map(int, p.split(":"))) for p in parts],) + tuple(map(int, marks.split()))
    return got


def test_cases_reach_what_a_map_can_get_wrong():
    tables = [(sum(blocks_of(s) for s, _, _ in c["items"]), sum(ceil_div(s, Q_TILE) for s, _, _ in c["items"])) for c in CASES]
    assert {1, 3} <= {rb for rb, _ in tables} and {1, 3} <= {t for _, t in tables}     # 4 and 12 bytes round to 8 and 16
    assert any(t % 2 == 0 and t for _, t in tables)                                   # ... and whole words stay
    assert any(c["cap"] == 0 for c in CASES) and any(c["tmp_bytes"] == 0 for c in CASES)
    assert any(sum(k for _, k, _ in c["items"]) == 0 for c in CASES)
    assert any(len(c["items"]) == 3 and (0, 0, 0) in c["items"] and c["items"][0] != (0, 0, 0) for c in CASES)
    assert CASES[0]["n_z"] == 1 and len(CASES[0]["items"]) == 1 and blocks_of(CASES[0]["items"][0][0]) == 1


def test_every_map_is_the_formula_written_out(built_maps):
    names, held = set(), 0
    for ci, c in enumerate(CASES):
        want = maps_of(c)
        names |= set(want)
        held += len(want)
        for name, (parts, uploaded, staged, total) in want.items():
            got = built_maps[ci, name]
            assert [at for at, _ in got[0]] == [at for at, _ in parts], (ci, name, "offsets", got, parts)
            assert [b for _, b in got[0]] == [b for _, b in parts], (ci, name, "part sizes")
            assert got[1:] == (uploaded, staged, total), (ci, name, "uploaded, staged, bytes", got[1:], (uploaded, staged, total))
    assert len(names) == 13 and len(built_maps) == 13 * len(CASES) and held >= 13 * (len(CASES) - 3)


def test_parts_start_on_8_bytes_and_never_overlap(built_maps):
    for key, (parts, uploaded, staged, total) in built_maps.items():
        assert uploaded <= staged <= total, key
        end = 0
        for i, (at, size) in enumerate(parts):
            assert at % 8 == 0 and at >= end and at - end < 8, (key, i)   # behind the part before it, with padding only between
            if size == 0 and i + 1 < len(parts):
                assert parts[i + 1][0] == at, (key, i)                    # a part of no bytes shares its start with the next
            end = at + size if size else end
        assert total == end, key
        assert uploaded in [0] + [at + size for at, size in parts] and staged in [0] + [at + size for at, size in parts], key
