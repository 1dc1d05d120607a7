"""Batches, the part that needs no device: how gfs_batch_plan cuts items into launches, the argument checks gfs_batch_create makes
before any device call, the exported symbols and structure sizes, and the planner compiled into a program of its own under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from util import ROOT
from gfasort_amd import hip

E_ARG, E_UNSUPPORTED = -1, -5


def test_plan_is_greedy_in_order():
    assert hip.batch_plan([5, 5, 5], 10) == ([0, 0, 1], 2)
    assert hip.batch_plan([5, 5], 10) == ([0, 0], 1)                   # an exact fit is taken
    assert hip.batch_plan([10, 10], 10) == ([0, 1], 2)
    assert hip.batch_plan([3, 7, 10, 1, 9, 1], 10) == ([0, 0, 1, 2, 2, 3], 4)   # in order: no item is moved to fill a gap
    assert hip.batch_plan([], 10) == ([], 0)
    assert hip.batch_plan([0, 0], 10) == ([0, 0], 1)
    with pytest.raises(hip.GfsError) as ei:
        hip.batch_plan([11], 10)
    assert ei.value.code == E_UNSUPPORTED and "item 0" in str(ei.value)
    with pytest.raises(hip.GfsError) as ei:
        hip.batch_plan([4, 4, 2 ** 63], 10)
    assert ei.value.code == E_UNSUPPORTED and "item 2" in str(ei.value)
    assert hip.batch_plan([2 ** 63, 2 ** 63, 1], 2 ** 64 - 1) == ([0, 1, 1], 2)   # a sum of 2^64 does not wrap into a fit
    L = hip.lib()
    n = C.c_uint32(7)
    assert L.gfs_batch_plan(None, 0, 10, None, C.byref(n)) == 0 and n.value == 0
    assert L.gfs_batch_plan(None, 1, 10, None, C.byref(n)) == E_ARG
    assert L.gfs_batch_plan(None, 0, 10, None, None) == E_ARG


def test_create_refuses_bad_arguments_before_any_device_call():
    L = hip.lib()
    h = C.c_void_p(1)
    one = (C.c_void_p * 1)(None)
    assert L.gfs_batch_create(None, 1, None, C.byref(h)) == E_ARG and h.value is None      # null list
    assert L.gfs_batch_create(one, 0, None, C.byref(h)) == E_ARG                           # n == 0
    assert L.gfs_batch_create(one, 1, None, None) == E_ARG and b"out" in L.gfs_last_error()
    assert L.gfs_batch_create(one, 1, None, C.byref(h)) == E_ARG and b"item 0" in L.gfs_last_error()   # a null entry
    with pytest.raises(hip.GfsError) as ei:
        hip.Batch([])
    assert ei.value.code == E_ARG
    assert L.gfs_batch_run(None, None) == E_ARG and L.gfs_batch_get_stats(None, None) == E_ARG
    L.gfs_batch_destroy(None)


def test_symbols_and_structure_sizes():
    L = hip.lib()
    for name in ("gfs_batch_plan", "gfs_batch_create", "gfs_batch_run", "gfs_batch_get_stats", "gfs_batch_destroy"):
        assert hasattr(L, name) and name in hip.EXPORTS, name
    assert C.sizeof(hip.BatchConfig) == 4 * 8
    assert C.sizeof(hip.BatchStats) == 8 * 8
    assert hip.BatchStats.kernel_ms.offset == 6 * 8


def test_rust_batch_structs_mirror_the_header_field_for_field():
    """INTEGRATION.md's GfsBatchConfig and GfsBatchStats against include/gfasort_hip.h: same names, order and widths."""
    import re
    from test_integration_doc import _c_structs, _docs, _rust_type_to_c
    rust, hdr = _docs()
    cs = _c_structs(hdr)
    for rname, cname in (("GfsBatchConfig", "gfs_batch_config"), ("GfsBatchStats", "gfs_batch_stats")):
        m = re.search(r"pub struct %s\s*\{(.*?)\}" % rname, rust, flags=re.S)
        assert m, f"INTEGRATION.md lacks {rname}"
        body = re.sub(r"//[^\n]*", "", m.group(1))
        got = []
        for f in body.split(","):
            f = f.strip()
            if f:
                name, rtype = re.match(r"pub (\w+)\s*:\s*(.+)$", f, flags=re.S).groups()
                got.append((name, _rust_type_to_c(rtype)))
        assert got == cs[cname], (rname, got, cs[cname])


SANITIZED_MAIN = r"""
#include "batch_plan.h"
#include <cstdio>
#include <vector>
static int failures = 0;
static void expect(const std::vector<uint64_t> &blocks, uint64_t max_blocks, uint64_t bad, const std::vector<uint32_t> &want, uint32_t n_want) {
    std::vector<uint32_t> got(blocks.size());                          // exactly n entries: one written past the end is caught
    uint32_t n = 99;
    const uint64_t r = gfs::batch_plan(blocks.data(), blocks.size(), max_blocks, got.data(), &n);
    if (r != bad || (bad == blocks.size() && (got != want || n != n_want))) { std::printf("case with %zu items failed\n", blocks.size()); ++failures; }
}
int main() {
    expect({5, 5, 5}, 10, 3, {0, 0, 1}, 2);
    expect({5, 5}, 10, 2, {0, 0}, 1);
    expect({10, 10}, 10, 2, {0, 1}, 2);
    expect({3, 7, 10, 1, 9, 1}, 10, 6, {0, 0, 1, 2, 2, 3}, 4);
    expect({}, 10, 0, {}, 0);
    expect({11}, 10, 0, {}, 0);
    expect({4, 4, 1ull << 63}, 10, 2, {}, 0);
    expect({1ull << 63, 1ull << 63, 1}, ~0ull, 3, {0, 1, 1}, 2);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_planner_under_sanitizers(tmp_path):
    """The planner (csrc/batch_plan.h, what gfs_batch_plan and gfs_batch_create call) in a stand-alone program built with
    -fsanitize=address,undefined, on the cases above."""
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "plan_main.cpp"
    src.write_text(SANITIZED_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
