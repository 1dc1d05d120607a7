"""The quality read-outs of a resident context (K7, quality_kernels.hip) on the GPU: positions are uploaded (the reference's
start plus seeded Gaussian noise) and measured; no test needs SGD to converge.

Bounds.  `pairs` and `max_rel_sq` are exact.  A sum of n non-negative doubles taken in two different orders differs by at most
n * 2^-52 relative (each of the at most n - 1 additions of either order rounds by <= 2^-53 relative to a partial sum that never
exceeds the total) — derived, not measured; the derived figures (a division and a square root on such sums) get 4 ulp more.

The pair kernel's grid is ceil(n_steps / 2048) workgroups (256 lanes x 8 pairs), at most 2048: the fixtures simple.gfa and
lil.gfa are fewer steps than one wave, DRB1-3123.gfa (35 059 steps) is 18 workgroups, and synth_bubbles(700, 8, 3) — 4 100+
steps — is the smallest of the generator's sizes tried here whose partials come from 3 workgroups."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from util import (O, G, P, DATA, load, oracle_graph, gaussian_init, graph_from_paths, self_loop_graph, absent_node_graph,
                  reverse_short_paths_graph)
from gfasort_amd import build as B
from gfasort_amd import hip, quality as Q
from gfasort_amd.layout import Layout
from quality_restatement import np_pair_errors, np_sort_quality, noisy_start

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")


def zero_length_graph():
    """Nodes of length 0 inside two paths: the step after such a node has the same bp position, d_path = 0, skipped."""
    lens = [3, 0, 2, 5, 0, 0, 4, 1, 2, 6]
    return graph_from_paths([[0, 1, 2, 3, 4, 5, 6, 7], [9, 4, 1, 8, 2, 0]], lens)


def tied_graph():
    """A chain of 300 nodes under three overlapping paths; its test positions are rounded to multiples of 40 bp (many ties)."""
    rng = np.random.default_rng(8)
    return graph_from_paths([list(range(0, 200)), list(range(100, 300)), list(range(50, 250))], rng.integers(1, 9, 300))


GRAPHS = {
    "simple": lambda: load("simple.gfa"), "lil": lambda: load("lil.gfa"), "DRB1": lambda: load("DRB1-3123.gfa"),
    "self_loop": self_loop_graph, "absent_node": absent_node_graph, "reverse_short_paths": reverse_short_paths_graph,
    "zero_length": zero_length_graph, "bubbles": lambda: G.synth_bubbles(700, 8, 3),
}
_cache = {}


def graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name]()
    return _cache[name]


def context(g, dims, positions=None, cfg=None, tweak=None):
    """A set-up context holding `positions` (no SGD is run)."""
    ctx = hip.Context(g)
    p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    if tweak:
        tweak(p)
    (ctx.setup_nd if dims else ctx.setup_1d)(p, cfg)
    if positions is not None:
        ctx.upload(positions)
    return ctx


def step_distances(g):
    longest = int(np.diff(g.path_first_step.astype(np.int64)).max())
    # the issue's list; then: longer than every path, z = n_steps, z far beyond n_steps
    return [1, 2, 3, 7, 64, 65, 1000, longest, g.n_steps, g.n_steps + 5, 1 << 40]


def assert_rows_match(g, coords, dims, rows):
    for r in rows:
        want = np_pair_errors(g, coords, dims, int(r["step_distance"]))
        n = want["pairs"]
        print(f"z={int(r['step_distance'])} pairs={int(r['pairs'])}/{n}",
              *(f"{k}: {float(r[k])!r} vs {want[k]!r}" for k in SUMS + ("max_rel_sq",)))
        assert int(r["pairs"]) == n
        assert float(r["max_rel_sq"]) == want["max_rel_sq"]
        for k in SUMS:
            assert abs(float(r[k]) - want[k]) <= n * U * abs(want[k]), (k, int(r["step_distance"]))


@pytest.mark.parametrize("dims", [0, 1, 2, 3, 8])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_pair_errors_equal_the_restatement(name, dims):
    g = graph(name)
    coords = noisy_start(g, dims, 17 + dims)
    ctx = context(g, dims, coords)
    zs = step_distances(g)
    rows = ctx.pair_errors(zs)
    assert rows["step_distance"].tolist() == zs
    if name == "bubbles":
        assert 2 * 2048 < g.n_steps <= 3 * 2048                         # 3 workgroups of partials
    assert_rows_match(g, coords, dims, rows)
    assert rows["pairs"][0] > 0 and not rows["pairs"][-4:].any() and not rows["sum_sq"][-4:].any()
    again = ctx.pair_errors(zs)
    assert rows.tobytes() == again.tobytes()                            # two calls: identical bits
    ctx.close()


def test_zero_length_nodes_are_skipped_where_the_path_distance_is_zero():
    g = graph("zero_length")
    ctx = context(g, 0, noisy_start(g, 0, 3))
    # adjacent pairs: 7 + 5; the pairs that START on a zero-length node (1, 4, 5 | 4, 1) have d_path = 0
    assert int(ctx.pair_errors([1])["pairs"][0]) == 12 - 5
    ctx.close()


def test_pair_errors_argument_and_state_errors():
    g = graph("lil")
    ctx = hip.Context(g)
    with pytest.raises(hip.GfsError) as ei:
        ctx.pair_errors([1])                                            # no positions yet
    assert ei.value.code == -4
    with pytest.raises(hip.GfsError) as ei:
        ctx.pair_errors([3, 0])
    assert ei.value.code == -1
    ctx.setup_1d(P.YgsParams.from_graph(g, 0, 1).path_sgd)
    assert ctx.pair_errors([]).shape[0] == 0
    with pytest.raises(hip.GfsError) as ei:
        ctx.stress_of_pairs([0], [g.n_steps])
    assert ei.value.code == -1
    ctx.close()


# ---- sampled stress: the reference's figure, from resident positions -------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2, 3, 8])
@pytest.mark.parametrize("name", ["simple", "lil", "DRB1"])
def test_sampled_stress_equals_the_oracle_bit_for_bit(name, dims):
    g = graph(name)
    og = oracle_graph(g)
    for coords in (noisy_start(g, dims, 5), gaussian_init(g, dims, 9) if dims else O.init_positions(og)):
        ctx = context(g, dims, coords)
        got = ctx.sampled_stress()
        want = O.layout_stress(og, dims, coords, 10000) if dims else O.stress_1d(og, coords, 10000)
        print(name, dims, repr(got), repr(want))
        assert got == want
        sa, sb = hip.stress_sample_pairs(g)
        stress, counted, rel = ctx.stress_of_pairs(sa, sb)
        assert stress == got and counted == int((rel >= 0).sum()) and np.all(rel[rel < 0] == -1.0)
        ctx.close()


# ---- sort quality ------------------------------------------------------------------------------------------------------------
def _tied_positions(g):
    return np.round(noisy_start(g, 0, 2, scale=30.0) / 40.0) * 40.0


@pytest.mark.parametrize("name,positions", [("DRB1", lambda g: noisy_start(g, 0, 4, scale=40.0)),
                                            ("absent_node", lambda g: noisy_start(g, 0, 4, scale=4.0)),
                                            ("tied", _tied_positions)])
def test_sort_quality_equals_the_integer_restatement(name, positions):
    g = tied_graph() if name == "tied" else graph(name)
    x = positions(g)
    if name == "tied":
        assert np.unique(x).shape[0] < g.n_nodes // 2
    ctx = context(g, 0, x)
    order = ctx.sort_order()
    assert np.array_equal(order, np.argsort(x, kind="stable").astype(np.uint64))
    q = ctx.sort_quality()
    want = np_sort_quality(g, order)
    print(q, want)
    for k in ("steps", "abs_err_sum", "genomic_sum"):
        assert q[k] == want[k], k
    n = want["steps"]
    assert n > 0 and abs(q["sq_err_sum"] - want["sq_err_sum"]) <= n * U * want["sq_err_sum"]
    ref = Q.layout_quality(g, order)
    assert ref["steps"] == n
    for k in ("rmse", "mae", "relative_error"):
        assert abs(q[k] - ref[k]) <= (n + 4) * U * abs(ref[k]), (k, q[k], ref[k])
    assert ctx.sort_quality() == q
    ctx.close()


def test_sort_quality_counts_an_absent_second_node_as_position_zero():
    g = graph("absent_node")
    sn = g.step_node.astype(np.int64)
    k = int(np.flatnonzero(sn == hip.NO_NODE)[0])
    assert k > 0 and sn[k - 1] != hip.NO_NODE                            # (node, absent): counted; (absent, node): skipped
    x = noisy_start(g, 0, 4, scale=4.0)
    ctx = context(g, 0, x)
    q, order = ctx.sort_quality(), ctx.sort_order()
    ctx.close()
    assert q["steps"] == g.n_steps - g.n_paths - 1
    spos = np.zeros(g.n_nodes, dtype=np.int64)
    spos[order.astype(np.int64)] = np.concatenate([[0], np.cumsum(g.node_len[order.astype(np.int64)].astype(np.int64))[:-1]])
    a = sn[k - 1]
    assert spos[a] > int(g.node_len[a])                                   # so that position 0 is visible in the sum
    other = np_sort_quality(g, order)
    assert q["abs_err_sum"] == other["abs_err_sum"]


def test_sort_quality_is_refused_on_a_layout_context():
    g = graph("lil")
    ctx = context(g, 2, noisy_start(g, 2, 1))
    with pytest.raises(hip.GfsError) as ei:
        ctx.sort_quality()
    assert ei.value.code == -4
    ctx.close()


# ---- a read-out between two launches changes nothing --------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_readout_between_launches_leaves_the_run_alone(dims):
    g = graph("DRB1")
    start = gaussian_init(g, dims, 3) if dims else None
    cfg = hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1))

    def small(p):
        p.iter_max, p.min_term_updates = 5, 3000

    def run(readout):
        ctx = context(g, dims, start, cfg, small)
        if not dims:
            ctx.init_positions()
        ctx.run_range([0, 1, 2])
        seen = None
        if readout:
            seen = (ctx.pair_errors([1, 2, 64]), ctx.sampled_stress(), Q.device_profile(ctx), ctx.sort_quality() if not dims else None)
        ctx.run_range([3, 4, 5])
        ctx.synchronize()
        x, st = ctx.download(), ctx.stats()
        ctx.close()
        return x, int(st.term_updates), seen
    x0, n0, _ = run(False)
    x1, n1, seen = run(True)
    assert n0 == n1 == 6 * 3000
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    assert seen[0]["pairs"][0] > 0 and seen[1] > 0.0


# ---- device_profile = the one-shot entry on the downloaded positions -----------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_device_profile_equals_the_one_shot_entry(dims):
    g = graph("DRB1")
    ctx = context(g, dims, noisy_start(g, dims, 21))
    rows = Q.device_profile(ctx)
    zs = Q.step_distance_ladder(int(np.diff(g.path_first_step.astype(np.int64)).max()))
    assert [r["z"] for r in rows] == zs and zs[:8] == [1, 2, 3, 4, 6, 8, 12, 16] and all(r["pairs"] > 0 for r in rows)
    resident = ctx.pair_errors(zs)
    one_shot = hip.pair_errors(g, ctx.download(), zs, dims)
    ctx.close()
    assert resident.tobytes() == one_shot.tobytes()
    assert rows == Q.profile_rows(one_shot)
    r0 = rows[0]
    assert r0["rms_rel"] == math.sqrt(float(one_shot["sum_rel_sq"][0]) / r0["pairs"]) and r0["max_rel"] == math.sqrt(float(one_shot["max_rel_sq"][0]))


# ---- CLI: --stress-profile ------------------------------------------------------------------------------------------------------
ROW = re.compile(r"^\[gfasort\] stress profile: z=(\d+) pairs=(\d+) rms_rel=(\S+) max_rel=(\S+) rmse_bp=(\S+) mae_bp=(\S+)$", re.M)


@pytest.fixture(scope="module")
def cli():
    B.build_host()
    return B.CLI


def assert_cli_rows(g, coords, dims, stderr):
    rows = ROW.findall(stderr)
    zs = Q.step_distance_ladder(int(np.diff(g.path_first_step.astype(np.int64)).max()))
    assert [int(r[0]) for r in rows] == zs and zs
    for z, pairs, rms_rel, max_rel, rmse, mae in rows:
        want = np_pair_errors(g, coords, dims, int(z))
        n = want["pairs"]
        assert int(pairs) == n and n > 0
        assert float(max_rel) == math.sqrt(want["max_rel_sq"])
        for got, ref in ((rms_rel, math.sqrt(want["sum_rel_sq"] / n)), (rmse, math.sqrt(want["sum_sq"] / n)), (mae, want["sum_abs"] / n)):
            print(z, got, repr(ref))
            assert abs(float(got) - ref) <= (n + 4) * U * abs(ref), (z, got, ref)


@pytest.mark.parametrize("name", ["lil.gfa", "DRB1-3123.gfa"])
def test_cli_stress_profile_after_a_layout(cli, tmp_path, name):
    o, tsv = str(tmp_path / "o.gfa"), str(tmp_path / "l.tsv")
    r = subprocess.run([cli, "-i", os.path.join(DATA, name), "-o", o, "-p", "L", "--dimensions", "2", "--layout-iter", "5",
                        "--layout-out", tsv, "--stress-profile", "-v", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = load(name)
    with open(tsv) as fh:
        lay = Layout.read_tsv(fh)
    assert (lay.dimensions, lay.num_nodes) == (2, g.n_nodes)
    assert_cli_rows(g, lay.coords, 2, r.stderr)
    # the -v line stays on the host function; the resident read-out gives the same figure to its printed digits
    printed = r.stderr.split("layout stress:")[1].split()[0]
    ctx = context(g, 2, lay.coords)
    assert "%.6f" % ctx.sampled_stress() == printed
    ctx.close()


@pytest.mark.parametrize("name,iters", [("lil.gfa", 100), ("DRB1-3123.gfa", 3)])
def test_cli_stress_profile_after_a_sort(cli, tmp_path, name, iters):
    o = str(tmp_path / "o.gfa")
    r = subprocess.run([cli, "-i", os.path.join(DATA, name), "-o", o, "-p", "Y", "--iter-max", str(iters), "--streams", "1",
                        "--stress-profile", "-v", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = load(name)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iters
    rc, x, _ = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1))
    assert rc == 0
    assert_cli_rows(g, x, 0, r.stderr)


def test_cli_without_the_flag_prints_no_profile(cli, tmp_path):
    o, tsv = str(tmp_path / "o.gfa"), str(tmp_path / "l.tsv")
    r = subprocess.run([cli, "-i", os.path.join(DATA, "lil.gfa"), "-o", o, "-p", "YL", "--dimensions", "2", "--layout-iter", "3",
                        "--iter-max", "5", "--layout-out", tsv, "-v", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "stress profile" not in r.stderr and "layout stress:" in r.stderr
