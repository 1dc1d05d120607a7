"""The batched diagnosis (K7h per path, K7i stretched pairs, K7j per node; batch_diagnosis_kernels.hip): gfs_batch_path_errors,
gfs_batch_stretched_pairs and gfs_batch_node_errors give, for every item of a batch of sorts or of layouts in a constant number of
launches, what gfs_ctx_path_errors, gfs_ctx_stretched_pairs and gfs_ctx_node_errors give one item at a time — field for field,
the doubles as bits — and touch nothing.

The batch.  Seven items whose tiles of 512 steps meet the seams of the flat tile space: a chain of 2048 steps (4 full tiles, no
partial one), lil (one tile: it shares a workgroup of four waves with its neighbours' tiles), a chain of 2049 steps (a last tile
of ONE step), DRB1 (69 tiles, 12 paths that begin inside tiles: tail partials), many_short (3000 paths of 2-5 steps, ~150
complete paths per tile, path ends on tile and round seams), hub (one path over 10 tiles from a tile's first step, every pair on
one node: K7j's contention case) and simple.  tests/test_batch_diagnosis_host.py holds the generators to these facts.

Positions.  `noisy`: noisy starts, iter_max = 2, one run() of the batch — the positions a batch leaves resident.  `shuffled`: the
shuffled starts as uploaded, not run, so that DRB1 at z = 1, ratio 10 has at least a quarter of its counted pairs stretched (the
reasoning of test_gpu_diagnosis.py's docstring holds for the start itself) and the list comparison is not vacuous.

Bounds.  Against the item's own call: every byte.  Against the restatement (quality_restatement.expected), test_gpu_diagnosis.py's
bounds: integers, max_rel_sq and listed pairs exact; a per-path sum of n non-negative doubles within n * 2^-52 relative."""
import ctypes as C
import re

import numpy as np
import pytest

from util import G, P, load, graph_from_paths, cli_solo_and_batch
from gfasort_amd import build, hip, quality as Q
from quality_restatement import expected, noisy_start, shuffled_start

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")
RATIOS = (10.0, 1.5)
NAMES = ("chain2048", "lil", "chain2049", "DRB1", "many_short", "hub", "simple")
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 7, -1.5, -2.5)


def _chain(n, seed):
    """One path over n nodes of lengths 1..16, whose S lines come in another order than the path visits them."""
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


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


_graphs = None


def graphs():
    global _graphs
    if _graphs is None:
        _graphs = [_chain(2048, 1), load("lil.gfa"), _chain(2049, 2), load("DRB1-3123.gfa"), many_short_graph(), hub_graph(),
                   load("simple.gfa")]
    return _graphs


def step_distances():
    return (1, 2, 65, 2048, max(g.n_steps for g in graphs()) + 5)


def _batch(dims, gs, kind="noisy", n_streams=0, run=True):
    """Set-up contexts holding `kind` start positions and their batch, after one run of the batch where asked for."""
    ctxs = []
    for i, g in enumerate(gs):
        ctx = hip.Context(g)
        p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
        p.iter_max = 2
        p.seed = 9399220 + i
        assert (ctx.setup_nd if dims else ctx.setup_1d)(p, hip.make_config(n_streams=n_streams)) == hip.OK
        ctx.upload(noisy_start(g, dims, 31 + i) if kind == "noisy" else shuffled_start(g, dims, 23 + dims + i))
        ctxs.append(ctx)
    b = hip.Batch(ctxs)
    if run:
        b.run()
    return ctxs, b


@pytest.fixture(scope="module", params=[(0, "noisy"), (2, "noisy"), (0, "shuffled"), (2, "shuffled")], ids=lambda p: f"dims{p[0]}-{p[1]}")
def resident(request):
    """(dims, kind, graphs, contexts, batch, coords per item), built once per kind and only read."""
    dims, kind = request.param
    gs = graphs()
    ctxs, b = _batch(dims, gs, kind, run=kind == "noisy")
    coords = [c.download() for c in ctxs]
    yield dims, kind, gs, ctxs, b, coords
    b.close()
    for c in ctxs:
        c.close()


def same_bits(a, b):
    """Field for field; the doubles compared as uint64."""
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a.dtype.names)


def test_batch_items_reach_their_seams():
    gs = graphs()
    assert [-(-g.n_steps // 512) for g in gs[:4]] == [4, 1, 5, 69] and gs[2].n_steps % 512 == 1 and -(-gs[5].n_steps // 512) == 10
    assert gs[4].n_paths == 3000 and 20 * 512 < gs[4].n_steps < 21 * 512 and gs[5].n_paths == 1 and gs[6].n_steps < 512
    first = gs[3].path_first_step.astype(np.int64)
    assert gs[3].n_paths == 12 and np.count_nonzero(first[1:-1] % 512) >= 10


# ---- 1: bit for bit the item's own call -----------------------------------------------------------------------------------------
def test_path_and_node_rows_are_the_items_own_bit_for_bit(resident):
    dims, kind, gs, ctxs, b, _ = resident
    assert b.path_offsets().tolist() == np.concatenate([[0], np.cumsum([g.n_paths for g in gs])]).tolist()
    for ratio in RATIOS:
        for z in step_distances():
            paths, pms = b.path_errors(z, ratio, return_ms=True)
            nodes, nms = b.node_errors(z, ratio, return_ms=True)
            assert len(paths) == len(nodes) == len(ctxs) and pms > 0.0 and nms > 0.0
            for i, c in enumerate(ctxs):
                assert paths[i].dtype == hip.PATH_ERROR_DTYPE and nodes[i].dtype == hip.NODE_ERROR_DTYPE
                assert same_bits(paths[i], c.path_errors(z, ratio)), (dims, kind, ratio, z, NAMES[i])
                assert same_bits(nodes[i], c.node_errors(z, ratio)), (dims, kind, ratio, z, NAMES[i])
    far = b.path_errors(step_distances()[-1], 10.0)
    assert not any(r["pairs"].any() for r in far) and all(int(r["steps"].sum()) == g.n_steps for r, g in zip(far, gs))
    at2048 = b.path_errors(2048, 10.0)
    assert int(at2048[0]["pairs"].sum()) == 0 and int(at2048[2]["pairs"].sum()) == 1 and int(at2048[3]["pairs"].sum()) > 1000


def test_stretched_pairs_are_the_items_own_bit_for_bit(resident):
    dims, kind, gs, ctxs, b, _ = resident
    n = len(ctxs)
    listed = 0
    for ratio in RATIOS:
        for z in step_distances():
            own = [c.stretched_pairs(z, ratio, cap=c.graph.n_steps + 1) for c in ctxs]          # (every pair of the item, its total)
            own_totals = [t for _, t in own]
            rows0, totals0 = b.stretched_pairs(z, ratio, cap=0)
            assert totals0.tolist() == own_totals and all(r.shape[0] == 0 for r in rows0)
            for cap in (max(own_totals) + 5, 7):
                out = np.zeros((n, cap), dtype=hip.STRETCHED_PAIR_DTYPE)
                out[:] = SENTINEL
                rows, totals = b.stretched_pairs(z, ratio, cap=cap, out=out)
                assert totals.tolist() == own_totals, (dims, kind, ratio, z, cap)
                for i in range(n):
                    k = min(cap, own_totals[i])
                    assert rows[i].shape[0] == k and same_bits(rows[i], own[i][0][:k]), (dims, kind, ratio, z, cap, NAMES[i])
                    assert np.all(out[i, k:] == np.array(SENTINEL, dtype=hip.STRETCHED_PAIR_DTYPE)), (dims, kind, ratio, z, cap, NAMES[i])
                    listed += k
            if kind == "shuffled" and z == 1 and ratio == 10.0:
                counted = int(ctxs[3].pair_errors([1])["pairs"][0])
                print("DRB1 shuffled: stretched", own_totals[3], "of", counted)
                assert 4 * own_totals[3] >= counted > 30000
    assert listed > 0


# ---- 2: against the restatement ---------------------------------------------------------------------------------------------------
def test_rows_match_the_restatement_and_each_other(resident):
    dims, kind, gs, ctxs, b, coords = resident
    for ratio in RATIOS:
        for z in step_distances():
            paths, nodes = b.path_errors(z, ratio), b.node_errors(z, ratio)
            cap = max(g.n_steps for g in gs)
            rows, totals = b.stretched_pairs(z, ratio, cap=cap)
            k7g = b.pair_errors([z])
            for i, g in enumerate(gs):
                want = expected(g, NAMES[i], dims, "batch-" + kind, coords[i], z, ratio)
                got, w = paths[i], want["paths"]
                print(NAMES[i], dims, kind, ratio, z, "pairs", int(got["pairs"].sum()), "stretched", int(got["stretched"].sum()))
                for k in ("steps", "reverse_steps", "pairs", "stretched", "max_rel_sq"):
                    assert np.array_equal(got[k], w[k]), (k, NAMES[i], dims, kind, ratio, z)
                for k in SUMS:
                    assert np.all(np.abs(got[k] - w[k]) <= w["pairs"] * U * np.abs(w[k])), (k, NAMES[i], dims, kind, ratio, z)
                for k in ("pairs", "stretched", "max_rel_sq"):
                    assert np.array_equal(nodes[i][k], want["nodes"][k]), (k, NAMES[i], dims, kind, ratio, z)
                assert int(totals[i]) == want["list"].shape[0] and rows[i].tobytes() == want["list"].tobytes()
                # the three read-outs and K7g agree
                assert int(got["pairs"].sum()) == int(k7g[i][0]["pairs"]) == want["counted"]
                assert int(got["stretched"].sum()) == int(totals[i])
                assert float(got["max_rel_sq"].max()) == (float(nodes[i]["max_rel_sq"].max()) if g.n_nodes else 0.0)
            if z == 1:
                assert int(nodes[5]["pairs"][0]) == 5000 and int(nodes[5]["stretched"][0]) == int(totals[5])    # the hub


# ---- 3: the grid ------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_grid(resident):
    dims, kind, gs, ctxs, b, _ = resident
    cap = max(g.n_steps for g in gs)

    def read(z, ratio):
        paths, nodes = b.path_errors(z, ratio), b.node_errors(z, ratio)
        rows, totals = b.stretched_pairs(z, ratio, cap=cap)
        return (b"".join(r.tobytes() for r in paths), b"".join(r.tobytes() for r in nodes), b"".join(r.tobytes() for r in rows),
                totals.tobytes())

    for z, ratio in ((1, 10.0), (65, 1.5)):
        want = read(z, ratio)
        assert read(z, ratio) == want                                    # a second call, the same bytes
        try:
            for blocks in (1, 2, 0):
                b.debug_tile_blocks(blocks)
                assert read(z, ratio) == want, (dims, kind, z, ratio, blocks)
        finally:
            b.debug_tile_blocks(0)


# ---- 4: nothing but the outputs is written -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_read_outs_leave_the_state_alone(dims):
    """Positions, counters and a following run() with the read-outs in between are those without them."""
    gs = [_chain(2049, 2), load("lil.gfa"), load("simple.gfa")]
    ctxs, b = _batch(dims, gs, n_streams=1)                              # one stream: a run is a function of its start
    plain, pb = _batch(dims, gs, n_streams=1)
    counters = lambda c: (c.stats().term_updates, c.stats().attempts, c.stats().iterations, c.stats().launches)
    before = [(c.download(), counters(c)) for c in ctxs]
    for z, ratio in ((1, 10.0), (2, 1.5)):
        b.path_errors(z, ratio)
        b.stretched_pairs(z, ratio, cap=64)
        b.node_errors(z, ratio)
    assert len(Q.batch_diagnosis(b)) == len(ctxs)
    for c, (x, st) in zip(ctxs, before):
        assert np.array_equal(c.download().view(np.uint64), x.view(np.uint64)) and counters(c) == st
    b.run()
    pb.run()
    for c, q in zip(ctxs, plain):
        assert np.array_equal(c.download().view(np.uint64), q.download().view(np.uint64)) and counters(c) == counters(q)
        assert counters(c)[2:] == (6, 2)
    b.close()
    pb.close()
    for c in ctxs + plain:
        c.close()


def test_batch_diagnosis_is_device_diagnosis_per_item(resident):
    dims, kind, gs, ctxs, b, _ = resident
    got = Q.batch_diagnosis(b, z=1, ratio=10.0, worst=3)
    assert got == [Q.device_diagnosis(c, z=1, ratio=10.0, worst=3) for c in ctxs]
    assert len(got[3]["rows"]) == 12 and len(got[3]["worst"]) == 3


# ---- 5: refusals, each before any write -------------------------------------------------------------------------------------------
def test_argument_rules_are_the_contexts():
    gs = [load("lil.gfa"), load("simple.gfa")]
    ctxs, b = _batch(0, gs, run=False)
    L, p = hip.lib(), hip._ptr
    n_paths, n_nodes = sum(g.n_paths for g in gs), sum(g.n_nodes for g in gs)
    po = np.zeros(n_paths + 1, dtype=hip.PATH_ERROR_DTYPE)
    no = np.zeros(n_nodes + 1, dtype=hip.NODE_ERROR_DTYPE)
    so = np.zeros((2, 4), dtype=hip.STRETCHED_PAIR_DTYPE)
    so[:] = SENTINEL
    totals = np.full(2, 77, dtype=np.uint64)
    off = np.zeros(3, dtype=np.uint64)
    untouched = lambda: (not po.view(np.uint64).any() and not no.view(np.uint64).any() and totals.tolist() == [77, 77] and
                         np.all(so == np.array(SENTINEL, dtype=hip.STRETCHED_PAIR_DTYPE)))
    path = lambda h, z, r, out, n: L.gfs_batch_path_errors(h, z, r, out, n, None, None)
    node = lambda h, z, r, out, n: L.gfs_batch_node_errors(h, z, r, out, n, None, None)
    pairs = lambda h, z, r, out, cap, t: L.gfs_batch_stretched_pairs(h, z, r, out, cap, t, None, None)
    assert path(None, 1, 10.0, p(po), n_paths) == E_ARG and node(None, 1, 10.0, p(no), n_nodes) == E_ARG
    assert pairs(None, 1, 10.0, p(so), 4, p(totals)) == E_ARG and L.gfs_batch_debug_tile_blocks(None, 1) == E_ARG
    assert L.gfs_batch_path_offsets(None, p(off), 3) == E_ARG and L.gfs_batch_path_offsets(b._h, None, 3) == E_ARG
    assert L.gfs_batch_path_offsets(b._h, p(off), 2) == E_ARG
    assert path(b._h, 1, 10.0, None, n_paths) == E_ARG and node(b._h, 1, 10.0, None, n_nodes) == E_ARG
    assert pairs(b._h, 1, 10.0, None, 4, p(totals)) == E_ARG and pairs(b._h, 1, 10.0, p(so), 4, None) == E_ARG
    for z, ratio, text in ((0, 10.0, b"step distance of 0"), (1, float("nan"), b"ratio"), (1, -1.0, b"ratio")):
        assert path(b._h, z, ratio, p(po), n_paths) == E_ARG and text in L.gfs_last_error()
        assert node(b._h, z, ratio, p(no), n_nodes) == E_ARG and text in L.gfs_last_error()
        assert pairs(b._h, z, ratio, p(so), 4, p(totals)) == E_ARG and text in L.gfs_last_error()
    assert path(b._h, 1, 10.0, p(po), n_paths + 1) == E_ARG and b"total_paths" in L.gfs_last_error()
    assert node(b._h, 1, 10.0, p(no), n_nodes - 1) == E_ARG and b"total_nodes" in L.gfs_last_error()
    assert untouched()
    # a context set up again for another kind since the batch was made: refused, the item named
    g = gs[1]
    assert ctxs[1].setup_nd(P.LayoutSGDParams.from_graph(g, 2, 1)) == hip.OK
    assert path(b._h, 1, 10.0, p(po), n_paths) == E_STATE and b"batch item 1" in L.gfs_last_error()
    assert node(b._h, 1, 10.0, p(no), n_nodes) == E_STATE and b"batch item 1" in L.gfs_last_error()
    assert pairs(b._h, 1, 10.0, p(so), 4, p(totals)) == E_STATE and b"batch item 1" in L.gfs_last_error()
    assert untouched()
    b.close()
    for c in ctxs:
        c.close()


def test_an_infinite_ratio_stretches_nothing_and_zero_everything(resident):
    dims, kind, gs, ctxs, b, _ = resident
    paths = b.path_errors(1, float("inf"))
    assert sum(int(r["pairs"].sum()) for r in paths) > 0 and not any(r["stretched"].any() for r in paths)
    _, totals = b.stretched_pairs(1, float("inf"), cap=3)
    assert not totals.any()


# ---- 6: the command line ----------------------------------------------------------------------------------------------------------
FIXTURES = ["simple.gfa", "lil.gfa", "DRB1-3123.gfa"]
DIAGNOSIS = re.compile(r"^\[gfasort\] diagnosis:.*$", re.M)


@pytest.mark.parametrize("step", ["Y", "L"])
def test_cli_batch_diagnose_prints_what_the_single_runs_print(tmp_path, step):
    build.build_host()
    flags = ["-p", step, "--streams", "1", "-v", "1", "--diagnose"] + (["--iter-max", "2"] if step == "Y" else ["--layout-iter", "1"])
    solo, r = cli_solo_and_batch(build.CLI, tmp_path, FIXTURES, flags, layouts=step == "L")
    assert all(s.returncode == 0 for s in solo), [s.stderr for s in solo]
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("in the batch") == len(FIXTURES), r.stderr
    assert f"[gfasort_hip] batch: diagnosis of {len(FIXTURES)} graphs read while resident\n" in r.stderr, r.stderr
    want = [line for s in solo for line in DIAGNOSIS.findall(s.stderr)]
    got = DIAGNOSIS.findall(r.stderr)
    assert len(want) > 3 * len(FIXTURES) and got == want
    quiet = cli_solo_and_batch(build.CLI, tmp_path, FIXTURES[:1], [f for f in flags if f != "--diagnose"], layouts=step == "L")[1]
    assert quiet.returncode == 0 and "diagnosis" not in quiet.stderr
