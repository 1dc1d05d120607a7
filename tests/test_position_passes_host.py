"""tests/position_passes_ref.py against pure-Python loops on tiny cases, and its inputs against what they claim to hold.  No GPU:
these are the restatements tests/test_gpu_position_passes.py holds reorder_positions_kernel, K4 and K6 to."""
import math
import struct

import numpy as np
import pytest

import position_passes_ref as R
from gfasort_amd.distributed import path_order_layout


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _word(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


@pytest.mark.parametrize("dims", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_device_order_restatement_equals_a_plain_loop(n, dims):
    perm = R.random_layout(n, 100 + n)
    w = 2 * dims if dims else 1
    v = R.abi_pattern(n, dims, tag=1)
    vb = [int(b) for b in _bits(v)]
    dev = [None] * (n * w)
    for k in range(n):                                                   # the rule as include/gfasort_hip.h and sgd_device.h state it
        if dims == 0:
            dev[int(perm[k])] = vb[k]
            continue
        for end in range(2):
            for dim in range(dims):
                dev[(end * dims + dim) * n + int(perm[k])] = vb[(k * 2 + end) * dims + dim]
    assert None not in dev and len(set(vb)) == len(vb)
    assert [int(b) for b in _bits(R.to_device(v, perm, dims))] == dev
    d = R.device_pattern(n, dims, tag=2)
    db = [int(b) for b in _bits(d)]
    abi = [None] * (n * w)
    for k in range(n):
        if dims == 0:
            abi[k] = db[int(perm[k])]
            continue
        for end in range(2):
            for dim in range(dims):
                abi[(k * 2 + end) * dims + dim] = db[(end * dims + dim) * n + int(perm[k])]
    assert [int(b) for b in _bits(R.to_abi(d, perm, dims))] == abi
    assert np.array_equal(_bits(R.to_abi(R.to_device(v, perm, dims), perm, dims)), _bits(v))
    special = set(int(s) for s in R._SPECIALS)
    assert (set(vb) - special).isdisjoint(db)                            # the two patterns share no mark


def test_patterns_name_their_elements_and_carry_the_specials():
    n, dims = 7, 3
    v, d = _bits(R.abi_pattern(n, dims, tag=1)), _bits(R.device_pattern(n, dims, tag=2))
    for pattern in (v, d):
        assert np.unique(pattern).shape[0] == pattern.shape[0]
        f = pattern.view(np.float64)
        assert np.isnan(f).sum() == 3 and np.isinf(f).sum() == 2 and (pattern == np.uint64(1) << np.uint64(63)).sum() == 1
        assert (pattern == 0).sum() == 1 and (pattern == 1).sum() == 1
    clean = _bits(R.abi_pattern(1, 3, tag=1))                            # (too short for the specials)
    assert [R.describe(b) for b in clean[[0, 4]]] == ["mark (index 0, end 0, dim 0) of pattern 1", "mark (index 0, end 1, dim 1) of pattern 1"]
    assert R.describe(R.marks(299, 0, 0, tag=9)) == "mark (index 299, end 0, dim 0) of pattern 9"
    assert R.describe(np.uint64(0xFFF8000000000123)).startswith("no mark: 0xfff8000000000123")


def test_first_difference_names_the_element_and_what_was_found():
    n, dims = 5, 3
    perm = R.random_layout(n, 3)
    v = R.abi_pattern(n, dims, tag=1)
    want = R.to_device(v, perm, dims)
    assert R.first_difference(want.copy(), want, "device", n, dims) is None
    r = (1 * dims + 2) * n                                               # swap two elements of plane (end 1, dim 2)
    got = want.copy()
    got[[r + 1, r + 3]] = got[[r + 3, r + 1]]
    text = R.first_difference(got, want, "device", n, dims)
    assert "D = 3" in text and "2 of 30" in text and "(end 1, dim 2, slot 1)" in text and "end 1, dim 2) of pattern 1" in text
    nan_a = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)
    nan_b = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)
    assert R.first_difference(nan_a, nan_a.copy(), "abi", 1, 0) is None  # bits, not values
    assert "no mark: 0x7ff8000000000000" in R.first_difference(nan_a, nan_b, "abi", 1, 0)


def test_prefix_restatement_equals_python_integers_past_2_53():
    lens = np.array([0, 0xFFFFFFFF, 3, 0, 0, 0xFFFFFFFF, 1, 0], dtype=np.uint32)
    total, want = 0, []
    for v in lens:
        want.append(float(total))
        total += int(v)
    assert np.array_equal(_bits(R.prefix_positions(lens)), _bits(np.array(want)))
    assert R.prefix_positions(np.zeros(0, np.uint32)).shape == (0,)
    # the conversion rounds to nearest, ties to even, as float(int) does: 2^53 + 1 -> 2^53, 2^53 + 3 -> 2^53 + 4
    sums = np.array([(1 << 53) + 1, (1 << 53) + 3, (1 << 63) + 1025], dtype=np.uint64)
    assert [_word(float(int(s))) for s in sums] == [int(b) for b in _bits(sums.astype(np.float64))]
    assert float((1 << 53) + 1) == float(1 << 53) and float((1 << 53) + 3) == float((1 << 53) + 4)
    # ... and on sums that get there: Python integers all the way, float() of each
    n = (1 << 21) + 2000
    lens = (0xFFFFFFFF - np.random.default_rng(1).integers(0, 2, n)).astype(np.uint32)
    exact = np.cumsum(lens.astype(object))
    tail = [0] + exact[:-1].tolist()
    assert R.prefix_sums(lens).tolist() == tail
    last = tail[-1500:]
    assert sum(s > 1 << 53 for s in last) > 1000 and sum(s & 1 for s in last) > 500
    assert [int(b) for b in _bits(R.prefix_positions(lens))[-1500:]] == [_word(float(s)) for s in last]
    assert sum(int(float(s)) != s for s in last) > 500                   # the conversion does round there


def test_sort_restatement_equals_a_stable_python_sort():
    x = R.hostile_positions(64, 5)
    x[:8] = [0.0, -0.0, 8.0, 8.0, -np.inf, np.inf, -8.0, 8.0]
    x[8:10] = np.array([0xFFF8000000000123, 0x7FF0000000000001], dtype=np.uint64).view(np.float64)

    def key(k):
        v = float(x[k])
        return (1, 0.0) if math.isnan(v) else (0, v)                     # (Python compares -0.0 == 0.0; sorted() is stable)
    want = sorted(range(64), key=key)
    got = R.sort_reference(x)
    assert got.dtype == np.uint64 and got.tolist() == want
    nans = [k for k in range(64) if math.isnan(float(x[k]))]
    assert want[-len(nans):] == nans and want[0] == 4


def test_hostile_positions_hold_what_the_sort_test_needs():
    x = R.hostile_positions(R.SEAM, 77)
    b = _bits(x)
    nan = np.isnan(x)
    assert (nan & (b >> np.uint64(63) == 1)).sum() >= 2 and (nan & (b >> np.uint64(63) == 0)).sum() >= 2
    assert np.unique(b[nan]).shape[0] >= 4
    assert (x == np.inf).any() and (x == -np.inf).any()
    assert (b == 0).sum() > 8 and (b == np.uint64(1) << np.uint64(63)).sum() > 8
    zeros = np.flatnonzero(x == 0.0)
    assert (np.diff(b[zeros].astype(np.int64) >> 63) != 0).sum() >= 8   # the two zeros alternate in dense order
    assert (x == 5e-324).any() and (x == -5e-324).any() and (x == 2.0 ** -1060).any() and (x < -8.0).any()
    assert np.unique(x[np.isfinite(x)]).shape[0] < R.SEAM // 8


def test_lengths_and_layouts_hold_what_they_claim():
    lens = R.mixed_lengths(R.SEAM, 5)
    zero = lens == 0
    assert zero[0] and zero[-1] and lens.max() == 16 and 0.1 < zero.mean() < 0.2 and (zero[1:] & zero[:-1]).sum() > 1000
    big = R.huge_lengths(10_000, 6)
    assert int(big[0]) == 0xFFFFFFFF and int(R.prefix_sums(big)[2]) > 1 << 32 and int(R.prefix_sums(big)[-1]) > 1 << 44
    for n in R.EDGE_SIZES:
        g = R.chain_under_two_paths(n, np.ones(n, np.uint32))
        assert g.n_paths == 2 and g.n_steps == 2 * n and g.n_nodes == n
        own = path_order_layout(g)
        perm = R.random_layout(n, 40 + n, avoid=(own,))
        assert sorted(perm.tolist()) == list(range(n))
        if n >= 2:
            assert not np.array_equal(perm, np.arange(n))
        if n >= 3:
            assert not np.array_equal(perm, own)
    g = R.chain_under_two_paths(1000, np.ones(1000, np.uint32), steps_per_path=2)
    assert g.path_step_counts().tolist() == [2, 2]
    assert not np.array_equal(path_order_layout(R.chain_under_two_paths(257, np.ones(257, np.uint32))), np.arange(257))
