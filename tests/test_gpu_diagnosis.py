"""The localising read-outs of a resident context (K7d per path, K7e stretched pairs, K7f per node; quality_kernels.hip) on the
GPU.  Positions are uploaded and measured; no SGD is run.  Expected values are the restatement's per-pair values
(quality_restatement.np_pairs_at / np_pair_values) grouped on the CPU per path and per node; d_layout = err + d_path and a
counted pair is stretched when d_layout / d_path > ratio, as the header states them.

Bounds.  Integer fields, max_rel_sq and every listed pair are exact.  A per-path sum of n non-negative doubles taken in two
different orders differs by at most n * 2^-52 relative — the bound derived in test_gpu_quality_readout.py's docstring — with
n the path's counted pairs.

Tiles.  K7d and K7e cut the step table into tiles of 512 steps, one wave each, 64 steps a round.  `many_short` (3000 paths of
2-5 steps, ~10 500 steps) puts ~150 paths into every tile and path ends on tile and round seams; `hub` is one path of 5001
steps over 10 tiles, begun at a tile's first step (a head partial in every tile); DRB1's 12 paths of ~2 900 steps start
inside tiles (tail partials).  The shuffled positions make a large share of the adjacent pairs stretched at ratio 10: with ~3.1k nodes averaging ~7 bp, two random nodes lie within 10 node lengths of each
other with probability around 1 %, so at least a quarter of the counted pairs must be — asserted before the list is compared."""
import os
import re
import subprocess

import numpy as np
import pytest

from util import G, P, DATA, load, graph_from_paths, self_loop_graph, absent_node_graph, reverse_short_paths_graph
from gfasort_amd import build as B
from gfasort_amd import hip, quality as Q
from quality_restatement import expected, noisy_start, shuffled_start

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")
DIMS = [0, 2, 8]


def zero_length_graph():
    lens = [3, 0, 2, 5, 0, 0, 4, 1, 2, 6]
    return graph_from_paths([[0, 1, 2, 3, 4, 5, 6, 7], [9, 4, 1, 8, 2, 0]], lens)


def many_short_graph():
    """3000 paths of 2-5 steps over 500 nodes, 30 % of the steps reverse."""
    rng = np.random.default_rng(11)
    paths = [rng.integers(0, 500, int(k)).tolist() for k in rng.integers(2, 6, 3000)]
    n = sum(len(p) for p in paths)
    return graph_from_paths(paths, rng.integers(1, 9, 500), rev=(rng.random(n) < 0.3))


def hub_graph():
    """One path h, a1, h, a2, ..., h of 5001 steps: every pair of adjacent steps touches node h (index 0)."""
    rng = np.random.default_rng(12)
    path = [0] * 5001
    path[1::2] = range(1, 2501)
    return graph_from_paths([path], rng.integers(1, 9, 2501))


GRAPHS = {
    "simple": lambda: load("simple.gfa"), "lil": lambda: load("lil.gfa"), "DRB1": lambda: load("DRB1-3123.gfa"),
    "self_loop": self_loop_graph, "absent_node": absent_node_graph, "reverse_short_paths": reverse_short_paths_graph,
    "zero_length": zero_length_graph, "bubbles": lambda: G.synth_bubbles(700, 8, 3),
    "many_short": many_short_graph, "hub": hub_graph,
}
_cache = {}


def graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name]()
    return _cache[name]


def context(g, dims, positions=None, node_perm=None):
    """A set-up context holding `positions` (no SGD is run)."""
    ctx = hip.Context(g, node_perm=node_perm)
    p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    (ctx.setup_nd if dims else ctx.setup_1d)(p)
    if positions is not None:
        ctx.upload(positions)
    return ctx


def step_distances(g):
    longest = int(np.diff(g.path_first_step.astype(np.int64)).max())
    return [1, 2, 65, longest, g.n_steps + 5]


def position_kinds(g, dims):
    noisy = noisy_start(g, dims, 17 + dims)
    return [("noisy", noisy, 1.5), ("noisy", noisy, 10.0), ("shuffled", shuffled_start(g, dims, 23 + dims), 10.0)]


def cases(name, dims):
    g = graph(name)
    for kind, coords, ratio in position_kinds(g, dims):
        for z in step_distances(g):
            yield kind, coords, ratio, z, expected(g, name, dims, kind, coords, z, ratio)


def by_kind(g, dims):
    """One context per kind of positions: (kind, coords, ctx)."""
    seen = {}
    for kind, coords, _ in position_kinds(g, dims):
        if kind not in seen:
            seen[kind] = (coords, context(g, dims, coords))
    return seen


def assert_shuffled_drb1_is_stretched(name, kind, z, ratio, want):
    if name == "DRB1" and kind == "shuffled" and z == 1:
        print("DRB1 shuffled: stretched", want["list"].shape[0], "of", want["counted"])
        assert ratio == 10.0 and 4 * want["list"].shape[0] >= want["counted"] > 30000


# ---- 1, 2: per path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_path_errors_equal_the_restatement_and_add_up_to_k7a(name, dims):
    g = graph(name)
    ctxs = by_kind(g, dims)
    for kind, coords, ratio, z, want in cases(name, dims):
        ctx = ctxs[kind][1]
        got = ctx.path_errors(z, ratio)
        w = want["paths"]
        print(name, dims, kind, ratio, z, "pairs", int(got["pairs"].sum()), "stretched", int(got["stretched"].sum()))
        for k in ("steps", "reverse_steps", "pairs", "stretched", "max_rel_sq"):
            assert np.array_equal(got[k], w[k]), (k, kind, ratio, z)
        for k in SUMS:
            assert np.all(np.abs(got[k] - w[k]) <= w["pairs"] * U * np.abs(w[k])), (k, kind, ratio, z)
        k7a = ctx.pair_errors([z])
        assert int(got["pairs"].sum()) == int(k7a["pairs"][0]) == want["counted"]
        assert float(got["max_rel_sq"].max()) == float(k7a["max_rel_sq"][0])
        assert got.tobytes() == ctx.path_errors(z, ratio).tobytes()      # two calls: identical bits
    z_long = step_distances(g)[3]
    assert not ctx.path_errors(z_long)["pairs"].any() and ctx.path_errors(1)["pairs"].sum() > 0
    for _, ctx in ctxs.values():
        ctx.close()


def test_tiles_of_the_fixtures_are_what_the_docstring_says():
    assert 20 * 512 < graph("many_short").n_steps < 21 * 512 and graph("many_short").n_paths == 3000
    assert graph("hub").n_steps == 5001 and graph("hub").n_paths == 1
    first = graph("DRB1").path_first_step.astype(np.int64)
    assert graph("DRB1").n_steps == 35059 and np.count_nonzero(first[1:-1] % 512) >= 10 and np.diff(first).min() > 2 * 512


# ---- 3: the list --------------------------------------------------------------------------------------------------------------
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 7, -1.5, -2.5)


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_stretched_pairs_are_the_restatements_in_step_order(name, dims):
    g = graph(name)
    ctxs = by_kind(g, dims)
    listed = 0
    for kind, coords, ratio, z, want in cases(name, dims):
        ctx = ctxs[kind][1]
        assert_shuffled_drb1_is_stretched(name, kind, z, ratio, want)
        w = want["list"]
        total = w.shape[0]
        got0, t0 = ctx.stretched_pairs(z, ratio, cap=0)                  # out = None
        assert t0 == total and got0.shape[0] == 0
        for cap in (7, total, total + 100):
            buf = np.zeros(cap + 3, dtype=hip.STRETCHED_PAIR_DTYPE)
            buf[:] = SENTINEL
            got, t = ctx.stretched_pairs(z, ratio, cap=cap, out=buf) if cap else ctx.stretched_pairs(z, ratio, cap=0)
            n = min(cap, total)
            print(name, dims, kind, ratio, z, "cap", cap, "total", t, "listed", got.shape[0])
            assert t == total and got.shape[0] == n
            assert got.tobytes() == w[:n].tobytes()                       # d_path and d_layout bit for bit
            assert np.all(buf[n:] == np.array(SENTINEL, dtype=hip.STRETCHED_PAIR_DTYPE))
            listed += n
        again, _ = ctx.stretched_pairs(z, ratio, cap=total + 100)
        assert again.tobytes() == w.tobytes()
    assert listed > 0 or name in ("simple", "lil", "zero_length", "absent_node", "self_loop")
    for _, ctx in ctxs.values():
        ctx.close()


# ---- 4: per node --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_node_errors_equal_the_restatement(name, dims):
    g = graph(name)
    ctxs = by_kind(g, dims)
    for kind, coords, ratio, z, want in cases(name, dims):
        ctx = ctxs[kind][1]
        got = ctx.node_errors(z, ratio)
        w = want["nodes"]
        for k in ("pairs", "stretched", "max_rel_sq"):
            assert np.array_equal(got[k], w[k]), (k, kind, ratio, z)
        assert got.tobytes() == ctx.node_errors(z, ratio).tobytes()
        if name == "hub" and z == 1:
            assert int(got["pairs"][0]) == want["counted"] == 5000
            assert int(got["stretched"][0]) == want["list"].shape[0]
    for _, ctx in ctxs.values():
        ctx.close()


def test_a_pair_from_a_node_to_itself_counts_once():
    g = graph("self_loop")
    sn = g.step_node.astype(np.int64)
    twice = np.flatnonzero(sn[:-1] == sn[1:])
    assert twice.shape[0] == 1                                            # 4+,4+
    node = int(sn[twice[0]])
    ctx = context(g, 0, noisy_start(g, 0, 3))
    got = ctx.node_errors(1, 10.0)
    ctx.close()
    # the node's adjacent pairs: (3-,4+), (4+,4+), (4+,5+) — three pairs, four ends on the node
    assert int(got["pairs"][node]) == 3
    assert int(got["pairs"].sum()) == 2 * (g.n_steps - 1) - 1


# ---- 5: determinism and purity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_readouts_leave_the_positions_alone_and_do_not_depend_on_the_node_layout(dims):
    g = graph("DRB1")
    coords = shuffled_start(g, dims, 5)
    ctx = context(g, dims, coords)
    paths, (pairs, total), nodes = ctx.path_errors(1, 10.0), ctx.stretched_pairs(1, 10.0, cap=50), ctx.node_errors(1, 10.0)
    assert np.array_equal(ctx.download().view(np.uint64), coords.view(np.uint64))
    default_perm = ctx.node_layout()
    ctx.close()
    perm = np.random.default_rng(9).permutation(g.n_nodes).astype(np.uint32)
    assert not np.array_equal(perm, default_perm)
    other = context(g, dims, coords, node_perm=perm)
    assert np.array_equal(other.node_layout(), perm)
    p2, (l2, t2), n2 = other.path_errors(1, 10.0), other.stretched_pairs(1, 10.0, cap=50), other.node_errors(1, 10.0)
    other.close()
    assert nodes.tobytes() == n2.tobytes() and pairs.tobytes() == l2.tobytes() and total == t2 > 50
    for k in ("steps", "reverse_steps", "pairs", "stretched", "max_rel_sq"):
        assert np.array_equal(paths[k], p2[k]), k
    assert paths.tobytes() == p2.tobytes()                                # the sums too: they do not read the layout either


# ---- 6: argument and state errors -----------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import ctypes as C
    g = graph("lil")
    L, p = hip.lib(), hip._ptr
    ctx = hip.Context(g)
    for call in (lambda: ctx.path_errors(1), lambda: ctx.stretched_pairs(1), lambda: ctx.node_errors(1)):
        with pytest.raises(hip.GfsError) as ei:
            call()                                                        # no positions yet
        assert ei.value.code == -4
    ctx.setup_1d(P.YgsParams.from_graph(g, 0, 1).path_sgd)
    ctx.upload(noisy_start(g, 0, 1))
    for z, ratio in ((0, 10.0), (1, float("nan")), (1, -1.0)):
        for call in (lambda: ctx.path_errors(z, ratio), lambda: ctx.stretched_pairs(z, ratio), lambda: ctx.node_errors(z, ratio)):
            with pytest.raises(hip.GfsError) as ei:
                call()
            assert ei.value.code == -1
    po = np.zeros(g.n_paths + 1, dtype=hip.PATH_ERROR_DTYPE)
    no = np.zeros(g.n_nodes + 1, dtype=hip.NODE_ERROR_DTYPE)
    so = np.zeros(4, dtype=hip.STRETCHED_PAIR_DTYPE)
    t = C.c_uint64(9)
    assert L.gfs_ctx_path_errors(ctx._h, 1, 10.0, p(po), g.n_paths + 1, None) == -1 and b"n_paths" in L.gfs_last_error()
    assert L.gfs_ctx_path_errors(ctx._h, 1, 10.0, None, g.n_paths, None) == -1
    assert L.gfs_ctx_node_errors(ctx._h, 1, 10.0, p(no), g.n_nodes - 1, None) == -1 and b"n_nodes" in L.gfs_last_error()
    assert L.gfs_ctx_node_errors(ctx._h, 1, 10.0, None, g.n_nodes, None) == -1
    assert L.gfs_ctx_stretched_pairs(ctx._h, 1, 10.0, None, 4, C.byref(t), None) == -1
    assert L.gfs_ctx_stretched_pairs(ctx._h, 1, 10.0, p(so), 4, None, None) == -1
    assert not po.view(np.uint64).any() and not no.view(np.uint64).any() and not so.view(np.uint64).any()
    rows = ctx.path_errors(1, float("inf"))                               # nothing is more than infinitely stretched
    assert rows["pairs"].sum() > 0 and not rows["stretched"].any()
    assert ctx.stretched_pairs(1, 0.0)[1] == int(rows["pairs"].sum())     # every counted pair has d_layout / d_path > 0 here
    ctx.close()


# ---- 7: one-shot, device_diagnosis, CLI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_one_shot_and_device_diagnosis_equal_the_context(dims):
    g = graph("DRB1")
    coords = shuffled_start(g, dims, 31)
    ctx = context(g, dims, coords)
    paths, (pairs, total) = ctx.path_errors(1, 10.0), ctx.stretched_pairs(1, 10.0, cap=64)
    diag = Q.device_diagnosis(ctx, worst=3)
    ctx.close()
    p1, l1, t1 = hip.diagnose(g, coords, 1, 10.0, cap=64, dims=dims)
    assert p1.tobytes() == paths.tobytes() and l1.tobytes() == pairs.tobytes() and t1 == total > 64
    _, l0, t0 = hip.diagnose(g, coords, 1, 10.0, cap=0, dims=dims)
    assert l0.shape[0] == 0 and t0 == total
    rms = np.sqrt(paths["sum_rel_sq"] / paths["pairs"])
    assert [r["rms_rel"] for r in diag["rows"]] == rms.tolist() and [r["stretched"] for r in diag["rows"]] == paths["stretched"].tolist()
    assert diag["worst"] == sorted(range(g.n_paths), key=lambda k: (-rms[k], k))[:3]


ROW = re.compile(r"^\[gfasort\] diagnosis:   (\S+): (\d+) steps, (\d+) forward, (\d+) reverse \((\S+)% reverse\), (\d+) pairs, "
                 r"rms relative error (\S+), (\d+) stretched$", re.M)


def test_cli_diagnose_prints_one_row_per_path(tmp_path):
    B.build_host()
    r = subprocess.run([B.CLI, "-i", os.path.join(DATA, "lil.gfa"), "-o", str(tmp_path / "o.gfa"), "-p", "Y", "--iter-max", "2",
                        "--diagnose"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = load("lil.gfa")
    rows = ROW.findall(r.stderr)
    first = g.path_first_step.astype(np.int64)
    assert [row[0] for row in rows] == list(g.path_names) and len(rows) == g.n_paths > 0
    for k, row in enumerate(rows):
        rev = int(g.step_is_rev[first[k]:first[k + 1]].sum())
        steps = int(first[k + 1] - first[k])
        assert (int(row[1]), int(row[2]), int(row[3])) == (steps, steps - rev, rev)
        assert int(row[5]) <= steps - 1 and float(row[6]) >= 0.0
    assert re.search(r"diagnosis: \d+ adjacent pairs with layout distance > 10 x path distance", r.stderr)
    quiet = subprocess.run([B.CLI, "-i", os.path.join(DATA, "lil.gfa"), "-o", str(tmp_path / "o2.gfa"), "-p", "Y", "--iter-max", "2"],
                           capture_output=True, text=True, timeout=120)
    assert quiet.returncode == 0 and "diagnosis" not in quiet.stderr
