"""Context sets (gfs_ctx_set_*, csrc/capi_set.hip) on the host: the arena plan, and every refusal gfs_ctx_set_create makes before
it touches a device.  No GPU needed; the build itself is held to gfs_ctx_create bit for bit in tests/test_gpu_ctx_set.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import load, graph_from_paths
from gfasort_amd import hip

E_ARG, E_HIP, E_UNSUPPORTED = -1, -2, -5
KIND_BYTES = (16, 16, 8, 4, 4)                     # step_rec, path_rec, path_len, perm, node_len


def _array_bytes(kind, n_nodes, n_steps, n_paths):
    return ((n_steps + 1) * 16, max(n_paths, 1) * 16, max(n_paths, 1) * 8, max(n_nodes, 1) * 4, max(n_nodes, 1) * 4)[kind]


def _create(views, n=None, device=0):
    """gfs_ctx_set_create over ctypes views (None entries stay null).  Returns (rc, handle value, error text)."""
    n = len(views) if n is None else n
    arr = (C.c_void_p * max(len(views), 1))(*[C.addressof(v) if v is not None else None for v in views])
    h = C.c_void_p(0xDEAD)                          # must be overwritten with NULL on failure
    rc = hip.lib().gfs_ctx_set_create(arr, C.c_uint64(n), C.c_int(device), C.byref(h))
    return rc, h.value, hip.lib().gfs_last_error().decode()


@pytest.mark.parametrize("counts", [
    [(0, 0, 0)],                                                        # a graph of nothing
    [(5, 0, 0)],                                                        # nodes, no paths
    [(3, 0, 2)],                                                        # two empty paths
    [(1, 1, 1)],                                                        # one step
    [(0, 0, 0), (12, 37, 5), (5, 0, 0), (1, 1, 1), (70001, 123457, 13), (64, 64, 64), (0, 0, 0), (63, 65, 1)],
])
def test_plan_aligned_disjoint_and_room_for_the_padding_record(counts):
    nn, ns, npth = ([c[k] for c in counts] for k in range(3))
    off, arena = hip.ctx_set_plan(nn, ns, npth)
    assert off.shape == (len(counts), 5)
    spans = []
    for i, (N, S, Pn) in enumerate(counts):
        for kind in range(5):
            begin = int(off[i, kind])
            assert begin % 256 == 0, (i, kind)
            spans.append((begin, begin + _array_bytes(kind, N, S, Pn)))
        assert _array_bytes(0, N, S, Pn) == (S + 1) * 16               # the + 1 record
    spans.sort()
    assert spans[0][0] == 0
    for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
        assert e0 <= b1, "arrays overlap"
    assert spans[-1][1] <= arena and arena % 256 == 0
    assert arena == sum((e - b + 255) // 256 * 256 for b, e in spans)  # nothing but the arrays and their alignment


def test_plan_refuses_null():
    L = hip.lib()
    one = np.ones(1, dtype=np.uint64)
    off, total = np.zeros(5, dtype=np.uint64), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.gfs_ctx_set_plan(None, p(one), p(one), 1, p(off), C.byref(total)) == E_ARG
    assert L.gfs_ctx_set_plan(p(one), p(one), p(one), 1, None, C.byref(total)) == E_ARG
    assert L.gfs_ctx_set_plan(p(one), p(one), p(one), 1, p(off), None) == E_ARG


def test_null_list_null_view_and_empty_list_are_argument_errors():
    v, keep = hip.make_view(load("simple.gfa"))
    L = hip.lib()
    h = C.c_void_p(0xDEAD)
    assert L.gfs_ctx_set_create(None, C.c_uint64(3), 0, C.byref(h)) == E_ARG and h.value is None
    assert L.gfs_ctx_set_create(None, C.c_uint64(0), 0, None) == E_ARG
    rc, handle, _ = _create([v], n=0)
    assert rc == E_ARG and handle is None
    rc, handle, why = _create([v, None, v])
    assert rc == E_ARG and handle is None and why.startswith("set item 1: ")


def _broken(g):
    """A view of g whose path_first_step does not end at n_steps."""
    first = np.array(g.path_first_step, dtype=np.uint64)
    first[-1] -= 1
    v, keep = hip.make_view(g)
    v.path_first_step = first.ctypes.data_as(C.c_void_p)
    return v, (keep, first)


def test_bad_path_first_step_names_its_item_and_the_lower_of_two():
    g = load("simple.gfa")
    good = [hip.make_view(g) for _ in range(5)]
    bad3, bad1 = _broken(g), _broken(g)
    views = [v for v, _ in good]
    views[3] = bad3[0]
    rc, handle, why = _create(views)
    assert rc == E_ARG and handle is None and why.startswith("set item 3: ") and "path_first_step" in why
    views[1] = bad1[0]
    rc, handle, why = _create(views)
    assert rc == E_ARG and handle is None and why.startswith("set item 1: ")
    # not monotone, in item 2 only
    first = np.array([0, 3, 2, 4], dtype=np.uint64)
    weird = graph_from_paths([[0, 1, 0], [1], [0]], [1, 2])
    v, keep = hip.make_view(weird)
    v.n_steps, v.path_first_step = 4, first.ctypes.data_as(C.c_void_p)
    rc, handle, why = _create([good[0][0], good[1][0], v])
    assert rc == E_ARG and handle is None and why.startswith("set item 2: ") and "monotone" in why


def _counts_only(n_nodes, n_steps, n_paths, first):
    """A view that is all counts: its arrays are one word each and must never be read past path_first_step[n_paths]."""
    word = np.zeros(2, dtype=np.uint64)
    ptr = word.ctypes.data_as(C.c_void_p)
    return hip.GraphView(n_nodes, n_steps, n_paths, ptr, ptr, ptr, first.ctypes.data_as(C.c_void_p)), word


def test_sums_past_one_contexts_limits_are_unsupported():
    zero = np.zeros(1, dtype=np.uint64)
    # nodes: three items of 2^30 nodes, no paths (each within its own limit)
    views = [_counts_only(1 << 30, 0, 0, zero) for _ in range(3)]
    rc, handle, why = _create([v for v, _ in views])
    assert rc == E_UNSUPPORTED and handle is None and "nodes" in why
    # steps: three items of one path of 2^39 steps
    first = np.array([0, 1 << 39], dtype=np.uint64)
    views = [_counts_only(1, 1 << 39, 1, first) for _ in range(3)]
    rc, handle, why = _create([v for v, _ in views])
    assert rc == E_UNSUPPORTED and handle is None and "steps" in why
    # paths: counts alone decide, path_first_step[2^30] is never looked at
    views = [_counts_only(1, 0, 1 << 30, zero) for _ in range(3)]
    rc, handle, why = _create([v for v, _ in views])
    assert rc == E_UNSUPPORTED and handle is None and "paths" in why
    # an item keeps its own limit, and is named
    views = [_counts_only(1, 0, 0, zero), _counts_only(1 << 31, 0, 0, zero)]
    rc, handle, why = _create([v for v, _ in views])
    assert rc == E_UNSUPPORTED and handle is None and why.startswith("set item 1: ")


def test_accessors_take_null():
    L = hip.lib()
    assert L.gfs_ctx_set_size(None) == 0
    assert L.gfs_ctx_set_item(None, 0) is None
    assert L.gfs_ctx_set_get_info(None, None) == E_ARG
    L.gfs_ctx_set_destroy(None)


@pytest.mark.skipif(hip.lib().gfs_device_count() > 0, reason="a GPU is present")
def test_valid_list_without_a_gpu_is_a_hip_error():
    views = [hip.make_view(load(name)) for name in ("simple.gfa", "lil.gfa")]
    rc, handle, why = _create([v for v, _ in views])
    assert rc == E_HIP and handle is None and "no CPU fallback" in why
    with pytest.raises(hip.GfsError) as ei:
        hip.ContextSet([load("simple.gfa")])
    assert ei.value.code == E_HIP


# ---- the planning arithmetic of the one driver (csrc/index_set_plan.h), in a program of its own -------------------------------------
SANITIZED_MAIN = r"""
#include "index_set_plan.h"
#include <cstdio>
#include <vector>

static int failures = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b, uint64_t c) {
    if (!ok) { std::printf("%s at N=%llu S=%llu P=%llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c); ++failures; }
}
static uint64_t up(uint64_t b) { return (b + 255) / 256 * 256; }

int main() {
    const uint64_t Ns[] = {0, 1, 63, 64, 65, 70001, 0x7FFFFFFFull}, Ss[] = {0, 1, 15, 16, 17, 255, 256, 257, 123457, 1ull << 40},
                   Ps[] = {0, 1, 31, 32, 33, 0x7FFFFFFFull};
    for (uint64_t N : Ns) for (uint64_t S : Ss) for (uint64_t P : Ps) {
        // the arena of a single context: a set of one item — exactly five offsets are written
        std::vector<uint64_t> off(gfs::SET_KINDS);
        const uint64_t arena = gfs::set_arena_plan(&N, &S, &P, 1, off.data());
        const uint64_t rec = up((S + 1) * 16), prec = up((P ? P : 1) * 16), plen = up((P ? P : 1) * 8), perm = up((N ? N : 1) * 4);
        expect(off[0] == 0 && off[1] == rec && off[2] == rec + prec && off[3] == rec + prec + plen && off[4] == rec + prec + plen + perm,
               "one-item offsets", N, S, P);
        expect(arena == rec + prec + plen + 2 * perm, "one-item arena", N, S, P);
        // the input head of one item and of seven: [step_node | path_first | item table | step_is_rev]
        for (uint64_t n : {1ull, 7ull}) {
            const gfs::SetInputHead h = gfs::set_input_head(S, P, n);
            expect(h.at_first == up(4 * S) && h.at_items == up(4 * S) + up(8 * (P + 1)) &&
                   h.at_rev == up(4 * S) + up(8 * (P + 1)) + up(64 * (n + 1)) && h.bytes == h.at_rev + up(S), "input head", N, S, P);
            expect(h.at_first % 256 == 0 && h.at_items % 256 == 0 && h.at_rev % 256 == 0 && h.bytes % 256 == 0, "input head alignment", N, S, P);
            expect(h.at_first >= 4 * S && h.at_items - h.at_first >= 8 * (P + 1) && h.at_rev - h.at_items >= 64 * (n + 1) && h.bytes - h.at_rev >= S,
                   "input head room", N, S, P);
        }
    }
    // two items: by kind, then by item, in arrays that hold exactly ten offsets
    const uint64_t nn[2] = {5, 0}, ns[2] = {0, 37}, np[2] = {0, 3};
    std::vector<uint64_t> off(2 * gfs::SET_KINDS);
    const uint64_t arena = gfs::set_arena_plan(nn, ns, np, 2, off.data());
    const uint64_t want[10] = {0, 1024, 1536, 2048, 2560, 256, 1280, 1792, 2304, 2816};
    for (int k = 0; k < 10; ++k) expect(off[k] == want[k], "two items", k, off[k], want[k]);
    expect(arena == 3072, "two items arena", arena, 0, 0);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """index_set_plan.h in a program of its own, built with -fsanitize=address,undefined (it is not loaded into Python): the arena
    of a single context — a set of one — and the input head in front of the build's scratch, against the formulas written out, at
    counts either side of the 256-byte alignment and at the limits of a context; the offset arrays hold exactly what is written."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "plan_main.cpp"
    src.write_text(SANITIZED_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "gfasort_amd", "csrc"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, (r.stdout, r.stderr)
