"""The quality read-outs' ABI (K7) on a machine WITHOUT a GPU: the new symbols are exported and listed, argument errors are
reported before any device call, the compute entries fail loudly, and gfs_stress_sample_pairs is the reference's sample stream:
its pairs, evaluated in plain Python floats and summed in order, give the oracle's stress bit for bit."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from util import O, ROOT, load, oracle_graph, gaussian_init
from gfasort_amd import hip, quality as Q
from quality_restatement import py_stress_of_pairs, noisy_start

NEW = ["gfs_ctx_pair_errors", "gfs_stress_sample_pairs", "gfs_ctx_stress_of_pairs", "gfs_ctx_sort_quality", "gfs_pair_errors"]
FIXTURES = ["simple.gfa", "lil.gfa", "DRB1-3123.gfa"]


def test_new_symbols_are_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "gfasort_hip.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = hip.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in hip.EXPORTS, name
    assert "typedef struct gfs_pair_error" in hdr and "typedef struct gfs_sort_quality" in hdr
    assert C.sizeof(hip.PairError) == 6 * 8 == hip.PAIR_ERROR_DTYPE.itemsize
    assert C.sizeof(hip.SortQuality) == 4 * 8
    assert [n for n, _ in hip.PairError._fields_] == list(hip.PAIR_ERROR_DTYPE.names)


def test_argument_errors_come_before_any_device_call():
    L = hip.lib()
    g = load("simple.gfa")
    v, keep = hip.make_view(g)
    x = hip.init_positions(g)
    out = np.zeros(2, dtype=hip.PAIR_ERROR_DTYPE)
    zs = np.array([1, 0], dtype=np.uint64)
    p = hip._ptr
    assert L.gfs_pair_errors(C.byref(v), 0, p(x), p(zs), 2, p(out)) == -1 and b"step distance of 0" in L.gfs_last_error()
    ok = np.array([1, 2], dtype=np.uint64)
    assert L.gfs_pair_errors(None, 0, p(x), p(ok), 2, p(out)) == -1
    assert L.gfs_pair_errors(C.byref(v), 0, p(x), None, 2, p(out)) == -1
    assert L.gfs_pair_errors(C.byref(v), 0, p(x), p(ok), 2, None) == -1
    assert L.gfs_pair_errors(C.byref(v), 0, None, p(ok), 2, p(out)) == -1
    assert L.gfs_pair_errors(C.byref(v), 9, p(x), p(ok), 2, p(out)) == -1
    # the context entries: a null context is an argument error
    cnt, st = C.c_uint64(0), C.c_double(0.0)
    assert L.gfs_ctx_pair_errors(None, p(ok), 2, p(out), None) == -1
    assert L.gfs_ctx_stress_of_pairs(None, p(ok), p(ok), 2, None, C.byref(cnt), C.byref(st)) == -1
    assert L.gfs_ctx_sort_quality(None, None) == -1
    n = C.c_uint64(0)
    assert L.gfs_stress_sample_pairs(None, 10, 1, p(ok), p(ok), C.byref(n)) == -1
    assert L.gfs_stress_sample_pairs(C.byref(v), 10, 1, None, p(ok), C.byref(n)) == -1
    assert L.gfs_stress_sample_pairs(C.byref(v), 10, 1, p(ok), p(ok), None) == -1


@pytest.mark.skipif(hip.lib().gfs_device_count() > 0, reason="a GPU is present")
def test_one_shot_fails_loudly_without_gpu():
    g = load("simple.gfa")
    with pytest.raises(hip.GfsError) as ei:
        hip.pair_errors(g, hip.init_positions(g), [1, 2])
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)
    with pytest.raises(hip.GfsError) as ei:
        hip.pair_errors(g, hip.init_layout(g, 2, 7), [1], dims=2)
    assert ei.value.code == -2


def test_ladder():
    assert Q.step_distance_ladder(100) == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96]
    assert Q.step_distance_ladder(13) == [1, 2, 3, 4, 6, 8, 12]
    assert Q.step_distance_ladder(4) == [1, 2, 3] and Q.step_distance_ladder(2) == [1]
    assert Q.step_distance_ladder(1) == [] and Q.step_distance_ladder(0) == []


def test_sample_pairs_stay_inside_their_path_and_handle_tiny_graphs():
    g = load("DRB1-3123.gfa")
    sa, sb = hip.stress_sample_pairs(g, 10000, 12345)
    assert 0 < sa.shape[0] <= 10000 and sa.shape == sb.shape
    first = g.path_first_step.astype(np.int64)
    pa = np.searchsorted(first, sa.astype(np.int64), side="right") - 1
    pb = np.searchsorted(first, sb.astype(np.int64), side="right") - 1
    assert np.array_equal(pa, pb) and np.all(sa != sb) and sa.max() < g.n_steps and sb.max() < g.n_steps
    a2, b2 = hip.stress_sample_pairs(g, 10000, 12345)
    assert np.array_equal(sa, a2) and np.array_equal(sb, b2)
    a3, _ = hip.stress_sample_pairs(g, 10000, 7)
    assert not np.array_equal(sa[:100], a3[:100])
    assert hip.stress_sample_pairs(g, 0)[0].shape[0] == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_sample_stream_is_the_oracles_1d(name):
    g = load(name)
    og = oracle_graph(g)
    sa, sb = hip.stress_sample_pairs(g, 10000, 12345)
    for x in (O.init_positions(og), noisy_start(g, 0, 11)):
        got, counted = py_stress_of_pairs(g, x, 0, sa, sb)
        want = O.stress_1d(og, x, 10000)
        assert got == want, (name, got, want, counted)
    assert counted > 0 and O.stress_1d(og, noisy_start(g, 0, 11), 10000) > 0.0


@pytest.mark.parametrize("dims", [2, 8])
@pytest.mark.parametrize("name", FIXTURES)
def test_sample_stream_is_the_oracles_layout(name, dims):
    g = load(name)
    og = oracle_graph(g)
    sa, sb = hip.stress_sample_pairs(g, 10000, 12345)
    for coords in (O.init_layout(og, dims, 9399220), gaussian_init(g, dims, 5)):
        got, counted = py_stress_of_pairs(g, coords, dims, sa, sb)
        want = O.layout_stress(og, dims, coords, 10000)
        assert got == want and counted > 0 and want > 0.0, (name, dims, got, want, counted)
