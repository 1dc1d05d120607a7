"""tests/test_gpu_readout_seams.py without a GPU: the seam graphs reach the seams they are named for, the restated reduction
tree is what its description says, and the comparisons the GPU file makes fail on the faults they are there to catch.  The
faults are injected into the restatement (quality_restatement.py), never into the product: a device that had one of them
would differ from the unfaulted restatement in the same figures."""
import functools
import math

import numpy as np
import pytest

from util import NO_NODE
from gfasort_amd import hip
import quality_restatement as R
from quality_restatement import (Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS, Q_TILE, quality_blocks_of, uncapped_blocks_of, seam_graph,
                                 noisy_start, shuffled_start, step_values, thread_sums, block_partials, grid_total, tree_sum,
                                 tree_count, tree_pair_errors, np_pair_errors, path_counts_from_tiles, grouped)

U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")


@functools.lru_cache(maxsize=None)
def graph(name):
    return seam_graph(name)


def _tiles_of(first, count):
    return (first + count - 1) // Q_TILE - first // Q_TILE + 1


# ---- 1: the graphs ------------------------------------------------------------------------------------------------------------
def test_the_restated_constants_and_record_types_are_the_products():
    assert (Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS) == (256, 8, 2048)
    assert [quality_blocks_of(n) for n in (0, 1, 2048, 2049, 524288, 524289, 4194304, 4194305, 1 << 40)] == \
        [1, 1, 1, 2, 256, 257, 2048, 2048, 2048]
    assert R.PATH_ERROR_DTYPE == hip.PATH_ERROR_DTYPE and R.STRETCHED_PAIR_DTYPE == hip.STRETCHED_PAIR_DTYPE
    assert R.NODE_ERROR_DTYPE == hip.NODE_ERROR_DTYPE


@pytest.mark.parametrize("name", ["medium", "medium-256"])
def test_medium_reaches_the_staging_and_the_combine_seams(name):
    g = graph(name)
    first = g.path_first_step.astype(np.int64)
    count = np.diff(first)
    # reduce_partials_kernel: one full staging tile of 256 partials and one entry more — or exactly one full tile
    if name == "medium":
        assert 256 * 2048 < g.n_steps <= 257 * 2048 and quality_blocks_of(g.n_steps) == 257
    else:
        assert g.n_steps == 256 * 2048 and quality_blocks_of(g.n_steps) == 256
    assert 15000 <= g.n_nodes <= 25000
    # path_combine_kernel: exactly one load of 64 tiles, head partials only
    assert first[0] == 0 and count[0] == 64 * Q_TILE and _tiles_of(first[0], count[0]) == 64
    # 65 tiles from a tile boundary: the second load has one tile
    assert first[1] % Q_TILE == 0 and _tiles_of(first[1], count[1]) == 65
    # at least 129 tiles from inside a tile: a tail partial at the first tile, three loads
    long_ = int(np.argmax(count))
    assert first[long_] % Q_TILE != 0 and _tiles_of(first[long_], count[long_]) >= 129
    # a stretch of short paths after a long one, over tile seams (every 512 steps) and round seams (every 64)
    short = np.flatnonzero((count >= 2) & (count <= 5))
    assert short.shape[0] >= 3000 and short.min() == 2 and np.all(np.diff(short[:3000]) == 1) and count[1] > 64 * Q_TILE
    over = lambda unit: int(np.count_nonzero(first[short] // unit != (first[short] + count[short] - 1) // unit))
    assert over(Q_TILE) >= 10 and over(64) >= 100
    # absent steps, reverse steps, zero-length nodes, a path without steps, a path of absent steps only
    absent = g.step_node == NO_NODE
    assert 500 < int(absent.sum()) < 2000 and 0.25 < g.step_is_rev.mean() < 0.35
    assert int(g.node_len.min()) == 0 and int(g.node_len.max()) == 8 and int((g.node_len == 0).sum()) > 1000
    assert int((count == 0).sum()) == 1 and count[-1] == 12 and absent[first[-2]:].all()
    # the combine takes one, two and at least three loads
    _, loads = path_counts_from_tiles(g, np.ones(g.n_steps))
    assert (loads == 1).sum() >= 5 and (loads == 2).sum() >= 5 and (loads >= 3).sum() >= 1
    # K7e: about a thousand tiles, so that the scan of the counts takes more than one block's worth
    assert -(-g.n_steps // Q_TILE) > 1000


def test_large_reaches_the_capped_grid_and_a_second_block_of_nodes():
    g = graph("large")
    per_pass = Q_MAX_BLOCKS * Q_BLOCK
    assert Q_MAX_BLOCKS * Q_BLOCK * Q_PAIRS_PER_THREAD < g.n_steps < Q_MAX_BLOCKS * Q_BLOCK * Q_PAIRS_PER_THREAD + 100000
    assert uncapped_blocks_of(g.n_steps) > quality_blocks_of(g.n_steps) == Q_MAX_BLOCKS
    for z in (1, 1000):                                         # some threads take 9 pairs, the others 8
        n = g.n_steps - z
        assert n // per_pass == Q_PAIRS_PER_THREAD and 0 < n % per_pass < per_pass
    assert 1024 * 256 < g.n_nodes <= 320000                     # the grid-stride step of the 1024 x 256 node kernels
    count = g.path_step_counts()
    assert count.max() <= 200000 and ((count >= 2) & (count <= 5)).sum() >= 5000
    assert -(-g.n_steps // Q_TILE) > 8000                       # K7e's scan over thousands of tile counts
    assert int((g.step_node == NO_NODE).sum()) > 1000 and int(g.node_len.min()) == 0


# ---- 2: the tree --------------------------------------------------------------------------------------------------------------
def _slow_tree(values, counted, n_steps):
    """The description of quality_restatement's tree as loops over threads, in Python floats."""
    B = quality_blocks_of(n_steps)
    n = len(values)
    partials = []
    for b in range(B):
        waves = []
        for w in range(Q_BLOCK // 64):
            lanes = []
            for l in range(64):
                acc, s = 0.0, b * Q_BLOCK + w * 64 + l
                while s < n:
                    if counted[s]:
                        acc = acc + values[s]
                    s += B * Q_BLOCK
                lanes.append(acc)
            for off in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
            waves.append(lanes[0])
        partials.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    total = 0.0
    for v in partials:
        total = total + v
    return total


def test_the_tree_is_its_description_on_three_workgroups():
    rng = np.random.default_rng(3)
    n_steps = 2 * 2048 + 700
    assert quality_blocks_of(n_steps) == 3
    for z in (1, 65):
        values = np.exp(rng.normal(0.0, 6.0, n_steps - z))      # fifteen orders of magnitude: the order of the adds shows
        counted = rng.random(n_steps - z) < 0.8
        got = tree_sum(values, counted, n_steps)
        assert got == _slow_tree(values.tolist(), counted.tolist(), n_steps)
        assert got != float(values[counted].sum()) or got != float(np.cumsum(values[counted])[-1])
        assert tree_count(counted, n_steps) == int(counted.sum())


@pytest.mark.parametrize("name", ["medium", "large"])
def test_the_tree_agrees_with_fsum_within_the_derived_bound(name):
    g = graph(name)
    v = step_values(g, noisy_start(g, 0, 17), 0, 1)
    n = int(v["counted"].sum())
    for k in ("rel", "abs", "sq"):
        exact = math.fsum(v[k][v["counted"]].tolist())
        got = tree_sum(v[k], v["counted"], g.n_steps)
        print(name, k, repr(got), repr(exact), abs(got - exact) / exact / U)
        assert abs(got - exact) <= n * U * exact


# ---- 3: the comparisons fail on injected faults ---------------------------------------------------------------------------------
def _differs_exactly(good, bad):
    """Which of the figures the GPU file compares exactly (pairs; the three sums as bits) a fault changes."""
    return [k for k in ("pairs",) + SUMS if good[k] != bad[k]]


def test_fault_partials_past_the_first_staging_tile_dropped():
    g = graph("medium")
    x = noisy_start(g, 0, 17)
    for z in (1, 64, 65, 1000):
        good = tree_pair_errors(g, x, 0, z)
        bad = tree_pair_errors(g, x, 0, z, staged=Q_BLOCK)
        assert good["pairs"] == np_pair_errors(g, x, 0, z)["pairs"]
        assert _differs_exactly(good, bad) == ["pairs"] + list(SUMS), z
    small = graph("medium-256")                                 # exactly one full staging tile: the fault does not show there
    xs = noisy_start(small, 0, 17)
    assert _differs_exactly(tree_pair_errors(small, xs, 0, 1), tree_pair_errors(small, xs, 0, 1, staged=Q_BLOCK)) == []


def test_fault_stride_taken_from_the_uncapped_grid():
    g = graph("large")
    x = noisy_start(g, 0, 17)
    wrong = uncapped_blocks_of(g.n_steps)
    for z in (1,):
        good = tree_pair_errors(g, x, 0, z)
        bad = tree_pair_errors(g, x, 0, z, stride_blocks=wrong)
        assert good["pairs"] == np_pair_errors(g, x, 0, z)["pairs"]
        assert _differs_exactly(good, bad) == ["pairs"] + list(SUMS), z
    m = graph("medium")                                         # under the cap the two grids are one: nothing to see
    assert uncapped_blocks_of(m.n_steps) == quality_blocks_of(m.n_steps)


def _k7d_integer_fields(g, coords, z, **fault):
    counted = np.zeros(g.n_steps, dtype=bool)
    counted[:max(g.n_steps - z, 0)] = step_values(g, coords, 0, z)["counted"]
    steps, loads = path_counts_from_tiles(g, np.ones(g.n_steps), **fault)
    pairs, _ = path_counts_from_tiles(g, counted, **fault)
    return steps, pairs, loads


@pytest.mark.parametrize("fault,hit", [(dict(max_tiles=64), lambda loads, inside: loads >= 2),
                                       (dict(swap_at_first_tile=True), lambda loads, inside: (loads >= 1) & inside)])
def test_fault_in_the_combine_changes_the_integer_fields_of_the_paths_it_touches(fault, hit):
    g = graph("medium")
    x = noisy_start(g, 0, 17)
    want = grouped(g, x, 0, 1, 10.0)["paths"]
    steps, pairs, loads = _k7d_integer_fields(g, x, 1)
    assert np.array_equal(steps, want["steps"].astype(np.int64)) and np.array_equal(pairs, want["pairs"].astype(np.int64))
    bad_steps, bad_pairs, _ = _k7d_integer_fields(g, x, 1, **fault)
    inside = g.path_first_step.astype(np.int64)[:-1] % Q_TILE != 0
    touched = hit(loads, inside)
    print(fault, "paths touched", int(touched.sum()), "steps wrong", int((bad_steps != steps).sum()), "pairs wrong", int((bad_pairs != pairs).sum()))
    assert touched.sum() >= 10
    # no other path, and every touched one — but for short paths whose two partials of 1-4 steps happen to be equal
    assert not (bad_steps != steps)[~touched].any() and (bad_steps != steps)[touched & (steps > 5)].all()
    assert (bad_steps != steps).sum() >= touched.sum() - 4
    assert not (bad_pairs != pairs)[~touched].any()
    # `pairs` of two partials can coincide where `steps` do not (skipped pairs): most touched paths, not every one
    assert 2 * int((bad_pairs != pairs)[touched].sum()) >= int(touched.sum())


def test_shuffled_positions_stretch_most_pairs_of_medium():
    g = graph("medium")
    e = grouped(g, shuffled_start(g, 0, 23), 0, 1, 10.0)
    assert e["counted"] > 400000 and 4 * e["list"].shape[0] >= e["counted"]
