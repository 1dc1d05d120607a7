"""Setup (gfs_ctx_set_setup_* and gfs_ctx_setup_*, csrc/capi_set.hip) on the host: the state arena's plan, the refusals made before
any device call, the zeta tables that items of like parameters share, the seeding kernel's tables for a set and for one item alone,
and the seeding rule the device kernel restates.  No GPU needed; the
setup itself is held to gfs_ctx_setup_* byte for byte in tests/test_gpu_set_setup.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import P, load, ROOT
from set_setup_ref import seeded_words, seeded_words_by_ints, MASK
from gfasort_amd import hip
from gfasort_amd import graph as G

E_ARG = -1
CSRC = os.path.join(ROOT, "gfasort_amd", "csrc")
# hand-made byte counts, item by item and kind by kind (positions, counters, team state, trace, trace counts, RNG, zetas, schedule):
# an item of nothing, one of positions only, sizes either side of the 256-byte alignment, a team item with traces
PLAN_CASES = [
    [[0] * 8],
    [[8 * 5, 0, 0, 0, 0, 0, 0, 0]],
    [[8 * 31, 65536, 0, 0, 0, 32 * 255, 8 * 31, 48 * 31], [0] * 8, [8 * 32, 65536, 0, 0, 0, 32 * 256, 8 * 32, 48 * 32],
     [8 * 33, 65536, 0, 0, 0, 32 * 257, 8 * 33, 48 * 33]],
    [[8 * 20000, 65536, 32 * 15040, 16 * 15040, 4 * 15040, 32 * 15040, 8 * 1000, 48 * 31], [8, 65536, 0, 16, 4, 32, 8 * 2, 48],
     [8 * 7, 0, 0, 0, 0, 0, 0, 0], [0] * 8, [8 * 4955, 65536, 0, 0, 0, 32 * 1216, 8 * 1002, 48 * 101]],
]


def test_the_five_symbols_are_exported():
    L = hip.lib()
    for name in ("gfs_ctx_set_state_plan", "gfs_ctx_set_setup_1d", "gfs_ctx_set_setup_nd", "gfs_ctx_set_get_setup_info", "gfs_ctx_debug_sgd_state"):
        assert hasattr(L, name) and name in hip.EXPORTS, name


@pytest.mark.parametrize("nbytes", PLAN_CASES)
def test_state_plan_aligned_adjacent_by_kind_and_disjoint(nbytes):
    off, arena = hip.ctx_set_state_plan(nbytes)
    n = len(nbytes)
    assert off.shape == (n, 8)
    spans, at = [], 0
    for kind in range(8):                                               # by kind, then by item: each array where the one before ends
        for i in range(n):
            begin, size = int(off[i, kind]), nbytes[i][kind]
            assert begin % 256 == 0, (i, kind)
            assert begin == at, (i, kind)
            at += (size + 255) // 256 * 256                             # an array of 0 bytes takes no room
            if size:
                spans.append((begin, begin + size))
    spans.sort()
    for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
        assert e0 <= b1, "arrays overlap"
    assert arena == at and arena % 256 == 0
    assert arena == (max(e for _, e in spans) + 255) // 256 * 256 if spans else arena == 0


def test_state_plan_refuses_null():
    L = hip.lib()
    nb, off, total = np.ones(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.gfs_ctx_set_state_plan(None, 1, p(off), C.byref(total)) == E_ARG
    assert L.gfs_ctx_set_state_plan(p(nb), 1, None, C.byref(total)) == E_ARG
    assert L.gfs_ctx_set_state_plan(p(nb), 1, p(off), None) == E_ARG and L.gfs_last_error() == b"null argument"
    assert L.gfs_ctx_set_state_plan(None, 0, None, C.byref(total)) == 0 and total.value == 0


def test_null_refusals_come_before_any_device_call():
    """A null set or null params is GFS_E_ARG with its text, on a machine with a device or without: nothing is dereferenced and
    no device call is made before the two checks (so a null set fails loudly where there is no GPU, too)."""
    L = hip.lib()
    sp, lp = hip.SgdParams(), hip.LayoutParams()
    rcs = np.zeros(1, dtype=np.int32)
    for entry, params in ((L.gfs_ctx_set_setup_1d, sp), (L.gfs_ctx_set_setup_nd, lp)):
        assert entry(None, C.byref(params), None, rcs.ctypes.data_as(C.c_void_p)) == E_ARG and L.gfs_last_error() == b"set is null"
        assert entry(None, None, None, None) == E_ARG and L.gfs_last_error() == b"set is null"
        not_a_set = C.create_string_buffer(4096)                        # never looked into: params is checked first
        assert entry(not_a_set, None, None, None) == E_ARG and L.gfs_last_error() == b"params is null"
    info = hip.ContextSetSetupInfo()
    assert L.gfs_ctx_set_get_setup_info(None, C.byref(info)) == E_ARG
    assert L.gfs_ctx_set_get_setup_info(C.create_string_buffer(64), None) == E_ARG and L.gfs_last_error() == b"null argument"
    word = C.c_uint64(0)
    assert L.gfs_ctx_debug_sgd_state(None, hip.STATE_RNG, C.byref(word), 8) == E_ARG and L.gfs_last_error() == b"ctx is null"


def _drb1_params():
    return P.YgsParams.from_graph(load("DRB1-3123.gfa"), 0, 1).path_sgd


def test_a_smaller_space_gives_a_prefix_of_the_larger_spaces_table():
    """What the shared zeta tables rest on (csrc/set_state_plan.h): with theta, space_max and the quantization step alike, the
    table of a smaller space is a prefix of the table of a larger one, bit for bit.  The helper itself is held to gfs_zeta_table of
    each item's own clamped parameters in the program below."""
    p = _drb1_params()
    p.space_max, p.space_quantization_step = 1000, 100
    tables = {}
    for space in (50, 3100, 15931):
        p.space = space
        tables[space] = hip.zeta_table(p)
    # sgd.rs:311-315: space + 1 up to space_max, else space_max + (space - space_max) / step + 1, + 1
    assert [len(tables[s]) for s in (50, 3100, 15931)] == [51, 1000 + 21 + 2, 1000 + 149 + 2]
    widest = tables[15931].view(np.uint64)
    for space in (50, 3100):
        own = tables[space].view(np.uint64)
        assert np.array_equal(own, widest[:len(own)]), space
    assert tables[50][50] > tables[50][49] > 0.0 and tables[3100][-1] > 0.0


@pytest.mark.parametrize("seed", [0, 9399220, (1 << 64) - 2])
@pytest.mark.parametrize("stream_base", [0, 5])
def test_numpy_seeding_is_the_rule_of_seed_streams(seed, stream_base):
    """Stream t <- four successive SplitMix64 outputs from seed + stream_base + t, wrapping at 2^64 (seed 2^64 - 2 wraps at
    t = 2, with stream_base 5 from the start): numpy's wrapping uint64 arrays against Python integers masked by hand, and against
    the one SplitMix64 the package already has."""
    T = 257
    got = seeded_words(seed, stream_base, T)
    assert got.dtype == np.uint64 and got.shape == (4 * T,)
    assert np.array_equal(got, seeded_words_by_ints(seed, stream_base, T))
    for t in (0, 1, 2, 3, 255, 256):
        own = G.splitmix64_array((seed + stream_base + t) & MASK, 4)
        assert np.array_equal(got[t::T], own), t
    if seed == 0 and stream_base == 0:                                  # SplitMix64(0): the published first outputs
        assert [int(v) for v in got[0::T][:3]] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


# ---- the plan and the zeta slices in a program of their own, under sanitizers -----------------------------------------------------
SANITIZED_MAIN = r"""
#include "set_state_plan.h"
#include "set_seed_tables.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static gfs_sgd_params params(double theta, uint64_t space, uint64_t space_max, uint64_t step) {
    gfs_sgd_params p;
    std::memset(&p, 0, sizeof p);
    p.iter_max = 30; p.min_term_updates = 1000; p.eps = 0.01; p.eta_max = 100.0; p.cooling_start = 0.5; p.seed = 9399220;
    p.theta = theta; p.space = space; p.space_max = space_max; p.space_quantization_step = step;
    return p;
}

int main() {
    using namespace gfs;
    // ---- the plan, over the inputs of the Python test, in arrays that hold exactly what is written ----
    const std::vector<std::vector<uint64_t>> cases = { PLAN_CASES };
    for (const std::vector<uint64_t> &bytes : cases) {
        const uint64_t n = bytes.size() / SET_STATE_KINDS;
        std::vector<uint64_t> off(bytes.size());
        const uint64_t arena = set_state_plan(bytes.data(), n, off.data());
        uint64_t at = 0;
        for (int kind = 0; kind < SET_STATE_KINDS; ++kind)
            for (uint64_t i = 0; i < n; ++i) {
                CHECK(off[SET_STATE_KINDS * i + kind] == at && at % 256 == 0);
                at += (bytes[SET_STATE_KINDS * i + kind] + 255) / 256 * 256;
            }
        CHECK(arena == at);
        CHECK(set_state_kind_begin(off.data(), GFS_STATE_POSITIONS) == 0);
        CHECK(set_state_kind_begin(off.data(), GFS_STATE_RNG) <= set_state_kind_begin(off.data(), GFS_STATE_ZETAS));
    }
    // ---- the clamp: the space a setup sums to, for the last staged index m = zlen_staged - 1 ----
    {
        const gfs_sgd_params p = params(0.99, 15931, 1000, 100);
        CHECK(zeta_clamped_space(p, 51) == 50);                          // m = 50 <= space_max: itself
        CHECK(zeta_clamped_space(p, 1001) == 1000);
        CHECK(zeta_clamped_space(p, 1002) == 1000);                      // m = space_max + 1: the sum at space_max
        CHECK(zeta_clamped_space(p, 1023) == 1000 + 21 * 100);           // m = space_max + 1 + 21
        CHECK(zeta_clamped_space(p, 1000000) == 15931);                  // never beyond the caller's space
        CHECK(zeta_clamped_space(p, 1) == 1);                            // at least 1
    }
    // ---- the slices: items that share (theta, space_max, step) at spaces 50, 3100 and 15931, an item of another key between
    // them, one that needs no table; each slice against gfs_zeta_table of the item's own clamped parameters, zero padding included
    {
        std::vector<gfs_sgd_params> clamped = {params(0.99, 3100, 1000, 100), params(0.99, 50, 1000, 100), params(0.5, 700, 1000, 100),
                                               params(0.99, 15931, 1000, 100), params(0.99, 9, 1000, 100), params(0.99, 3100, 1000, 10),
                                               params(0.99, 1000, 1000, 100), params(0.99, 1001, 1000, 100)};
        std::vector<uint8_t> needed(clamped.size(), 1);
        needed[4] = 0;
        const SharedZetaTables shared = shared_zeta_tables(clamped.data(), needed.data(), clamped.size());
        CHECK(shared.tables.size() == 3);
        CHECK(shared.table_of[0] == shared.table_of[1] && shared.table_of[0] == shared.table_of[3] && shared.table_of[0] == shared.table_of[6] &&
              shared.table_of[0] == shared.table_of[7]);
        CHECK(shared.table_of[2] != shared.table_of[0] && shared.table_of[5] != shared.table_of[0] && shared.table_of[5] != shared.table_of[2]);
        for (size_t i = 0; i < clamped.size(); ++i) {
            if (!needed[i]) continue;
            gfs_sgd_params full = clamped[i];
            full.space = 15931;                                           // the caller's space: what zlen_full comes from
            for (uint64_t zlen_full : {gfs_zeta_table_len(&full), gfs_zeta_table_len(&clamped[i]), gfs_zeta_table_len(&clamped[i]) - 1}) {
                std::vector<double> got(zlen_full, 0.0), want(zlen_full, 0.0), own(gfs_zeta_table_len(&clamped[i]));
                zeta_slice(shared.tables[shared.table_of[i]], clamped[i], zlen_full, got.data());
                CHECK(gfs_zeta_table(&clamped[i], own.data()) == GFS_OK);
                std::memcpy(want.data(), own.data(), std::min<size_t>(own.size(), want.size()) * sizeof(double));
                CHECK(std::memcmp(got.data(), want.data(), zlen_full * sizeof(double)) == 0);
                CHECK(zlen_full < 3 || got[2] > got[1]);                  // (a table, not zeros)
            }
        }
        // nothing needed: no table is summed
        std::vector<uint8_t> none(clamped.size(), 0);
        CHECK(shared_zeta_tables(clamped.data(), none.data(), clamped.size()).tables.empty());
        CHECK(shared_zeta_tables(nullptr, nullptr, 0).tables.empty());
    }
    // ---- the seeding tables behind the state arrays (set_seed_tables.h), in a mirror that holds exactly their range: a set of
    // items of 255, 256, 257, 1 and 70000 streams, and the set of one that a single context is
    {
        struct Item { uint64_t *rng; uint64_t first; uint32_t n_streams, first_block; };
        static_assert(sizeof(Item) == 24, "as set_seed.h SeedItem");
        const uint32_t B = 256;
        for (const std::vector<uint32_t> &streams : std::vector<std::vector<uint32_t>>{{255, 256, 257, 1, 70000}, {257}, {1}}) {
            std::vector<Item> items;
            uint64_t total = 0, most = 0;
            for (uint32_t T : streams) {
                const uint64_t nb = (T + B - 1) / B;
                items.push_back(Item{reinterpret_cast<uint64_t *>(uintptr_t(0x1000 * (items.size() + 1))), 7 + T, T, (uint32_t)total});
                total += nb; most = std::max(most, nb);
            }
            const uint64_t begin = 256 * 5;
            const SeedTables t = seed_tables_plan(begin, items.size(), sizeof(Item), total, most);
            CHECK(t.items_at == begin && t.blocks_at % 256 == 0 && t.alone_at % 256 == 0 && t.zeros_at % 256 == 0 && t.end % 256 == 0);
            CHECK(t.blocks_at - t.items_at >= items.size() * sizeof(Item) && t.alone_at - t.blocks_at >= total * 4);
            CHECK(t.zeros_at - t.alone_at >= items.size() * sizeof(Item) && t.end - t.zeros_at >= most * 4);
            std::vector<unsigned char> mirror(t.end - begin, 0);
            fill_seed_tables(t, items.data(), items.size(), B, mirror.data());
            const uint32_t *block_item = reinterpret_cast<const uint32_t *>(mirror.data() + (t.blocks_at - begin));
            const uint32_t *zeros = reinterpret_cast<const uint32_t *>(mirror.data() + (t.zeros_at - begin));
            uint64_t b = 0;
            for (size_t k = 0; k < items.size(); ++k) {
                Item all, alone;
                std::memcpy(&all, mirror.data() + k * sizeof(Item), sizeof(Item));
                std::memcpy(&alone, mirror.data() + (t.alone_at - begin) + k * sizeof(Item), sizeof(Item));
                CHECK(std::memcmp(&all, &items[k], sizeof(Item)) == 0);
                CHECK(alone.rng == items[k].rng && alone.first == items[k].first && alone.n_streams == items[k].n_streams && alone.first_block == 0);
                const uint64_t nb = (items[k].n_streams + B - 1) / B;
                CHECK(all.first_block == b);
                for (uint64_t j = 0; j < nb; ++j, ++b) CHECK(block_item[b] == k);   // every workgroup of the launch over all finds its item
                for (uint64_t j = 0; j < nb; ++j) CHECK(zeros[j] == 0);            // ... and every workgroup of the item's own launch item 0
            }
            CHECK(b == total);
        }
        const SeedTables none = seed_tables_plan(512, 0, sizeof(Item), 0, 0);       // nothing to do: no room
        CHECK(none.end == 512);
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_and_zeta_slices_under_sanitizers(tmp_path):
    """set_state_plan.h in a program of its own, host_tables.hip beside it as plain C++ (gfs_zeta_table), built with
    -fsanitize=address,undefined and run here; nothing of it is loaded into Python."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cases = ", ".join("{" + ", ".join(str(v) for item in case for v in item) + "}" for case in PLAN_CASES)
    src = tmp_path / "set_state_main.cpp"
    src.write_text(SANITIZED_MAIN.replace("PLAN_CASES", cases))
    exe = tmp_path / "set_state_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), str(src), "-x", "c++", os.path.join(CSRC, "host_tables.hip")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
