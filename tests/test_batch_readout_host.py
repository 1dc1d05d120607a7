"""The batch read-out (K4b / K6b), the part that needs no device: the exported symbols, the argument checks made before any device
call, and the sorting network's arithmetic (csrc/segment_sort.h, what the kernel takes every index and decision from) run serially
in a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

from util import ROOT
from gfasort_amd import hip

E_ARG = -1
NAMES = ("gfs_batch_result_offsets", "gfs_batch_init_positions", "gfs_batch_results", "gfs_batch_debug_sort_cap")


def test_symbols_are_exported_and_listed():
    L = hip.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hip.EXPORTS, name
    for method in ("result_offsets", "init_positions", "results", "debug_sort_cap"):
        assert callable(getattr(hip.Batch, method))
    hdr = open(os.path.join(ROOT, "include", "gfasort_hip.h")).read()
    assert "#define GFS_SEGMENT_SORT_CAP %d" % hip.SEGMENT_SORT_CAP in hdr
    assert hip.SEGMENT_SORT_CAP >= 4955                                 # DRB1-3123 is sorted in LDS


def test_null_batch_is_refused_without_a_device():
    L = hip.lib()
    off = (C.c_uint64 * 2)()
    x = (C.c_double * 1)()
    o = (C.c_uint32 * 1)()
    assert L.gfs_batch_result_offsets(None, off, 2) == E_ARG
    assert L.gfs_batch_init_positions(None, None) == E_ARG
    assert L.gfs_batch_results(None, x, o, 1, None, None) == E_ARG
    assert L.gfs_batch_debug_sort_cap(None, 64) == E_ARG
    assert b"null" in L.gfs_last_error()


SANITIZED_MAIN = r"""
#include "segment_sort.h"
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>
static int failures = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void run(const char *what, const std::vector<uint64_t> &in) {
    const uint32_t n = (uint32_t)in.size(), padded = gfs::segment_padded(n);
    if (padded < n || padded < gfs::SEGMENT_WAVE || (padded & (padded - 1)) || (padded >= 2 * gfs::SEGMENT_WAVE && padded / 2 >= n)) {
        std::printf("%s n=%u: padded length %u\n", what, n, padded); ++failures; return;
    }
    // exactly `padded` elements each: a partner out of range is a heap overflow
    std::vector<uint64_t> keys(padded), scratch_keys(padded);
    std::vector<uint32_t> index(padded), scratch_index(padded);
    std::copy(in.begin(), in.end(), keys.begin());
    std::iota(index.begin(), index.begin() + n, 0u);
    gfs::segment_sort_serial(keys.data(), index.data(), n, padded, scratch_keys.data(), scratch_index.data());
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return in[a] < in[b]; });
    bool ok = true;
    for (uint32_t r = 0; r < n; ++r) ok = ok && index[r] == want[r] && keys[r] == in[want[r]];
    for (uint32_t r = n; r < padded; ++r) ok = ok && index[r] == gfs::SEGMENT_PAD_INDEX && keys[r] == gfs::SEGMENT_PAD_KEY;
    if (!ok) { std::printf("%s n=%u: not the stable order\n", what, n); ++failures; }
}

static void cases(uint32_t n) {
    std::vector<uint64_t> v(n);
    for (auto &k : v) k = next();
    run("random", v);
    for (auto &k : v) k = next() % 7;                                  // runs of equal values, in no order
    run("few values", v);
    for (uint32_t i = 0; i < n; ++i) v[i] = i / 5;                     // runs of equal values, sorted
    run("equal runs", v);
    std::fill(v.begin(), v.end(), 42ull);
    run("all equal", v);
    for (uint32_t i = 0; i < n; ++i) v[i] = 3ull * i;
    run("sorted", v);
    for (uint32_t i = 0; i < n; ++i) v[i] = 3ull * (n - i);
    run("reversed", v);
    std::fill(v.begin(), v.end(), gfs::SEGMENT_PAD_KEY);               // NaNs only: the padding's key, below it by index
    run("all ones", v);
    for (uint32_t i = 0; i < n; ++i) v[i] = (i % 3 == 1) ? gfs::SEGMENT_PAD_KEY : next() % 4;
    run("all ones mixed in", v);
}

int main() {
    for (uint32_t n = 1; n <= 130; ++n) cases(n);
    for (uint32_t n : {255u, 256u, 257u, 1000u, 8192u}) cases(n);
    if (gfs::segment_padded(gfs::SEGMENT_SORT_CAP) != gfs::SEGMENT_SORT_CAP || gfs::segment_lds_bytes(gfs::SEGMENT_SORT_CAP) != 96u * 1024u) {
        std::printf("cap\n"); ++failures;
    }
    for (uint32_t p = gfs::SEGMENT_WAVE; p <= gfs::SEGMENT_SORT_CAP; p <<= 1) {
        const uint32_t b = gfs::segment_block(p);                      // whole waves, no thread without an element
        if (b % 64 || b > 1024 || b > p || p % b) { std::printf("block of %u\n", p); ++failures; }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_network_schedule_under_sanitizers(tmp_path):
    """segment_sort.h's schedule, serially, against std::stable_sort by key, for every n in 1..130 and 255, 256, 257, 1000, 8192,
    built with -fsanitize=address,undefined; the arrays hold exactly the padded length."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "segment_main.cpp"
    src.write_text(SANITIZED_MAIN)
    exe = tmp_path / "segment_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
