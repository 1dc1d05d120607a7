"""Context sets on the device (gfs_ctx_set_*, csrc/capi_set.hip, K3b in csrc/index_set_kernels.hip): every item of a set built
in one pass over the disjoint union of its graphs holds, bit for bit, what gfs_ctx_create gives for that graph alone — the index
build is integer arithmetic, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

from util import G, P, load, graph_from_paths, gaussian_init, absent_node_graph, self_loop_graph, reverse_short_paths_graph, \
    crowding_edge_graph, NO_NODE
from index_ref import HostIndex, free_device_bytes as _free_bytes
from gfasort_amd import hip
from gfasort_amd import sgd as S

pytestmark = pytest.mark.gpu

E_ARG = -1
ONE_STREAM = dict(n_streams=1)
# the grids of index_set_kernels.hip (index_set.h): threads of one grid-stride pass
STEP_PASS, NODE_PASS, PATH_PASS = 2048 * 256, 1024 * 256, 64 * 256


def _ygs(g, iter_max=10, updates=3000):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _layout_params(g, dims=2, iter_max=10, updates=3000):
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _empty_first_path_graph():
    """First path empty, an empty path between two others, nodes 3 and 4 (the middle of the index range) never visited."""
    return graph_from_paths([[], [5, 6, 0, 1], [], [1, 2, 7, 0, 5]], [3, 1, 4, 1, 5, 9, 2, 6], rev=[0, 1, 0, 0, 1, 1, 0, 0, 1])


def _hostile_mix():
    return [load("simple.gfa"), absent_node_graph(), graph_from_paths([], [2, 3, 5, 7, 11]), graph_from_paths([], []),
            load("lil.gfa"), self_loop_graph(), reverse_short_paths_graph(), crowding_edge_graph()[0], _empty_first_path_graph(),
            G.synth_bubbles(40, 7, 3), load("DRB1-3123.gfa"), load("simple.gfa")]


@pytest.fixture(scope="module")
def mix():
    """The hostile mix as one set and as solo contexts, nothing set up yet; shared and closed at the end."""
    graphs = _hostile_mix()
    cset = hip.ContextSet(graphs)
    solos = [hip.Context(g) for g in graphs]
    yield graphs, cset, solos
    for c in solos:
        c.close()
    cset.close()


def _outcome(fn):
    """What a call gives, comparable: its bytes, or the library's error code."""
    try:
        out = fn()
        return ("ok", out.tobytes() if isinstance(out, np.ndarray) else out)
    except hip.GfsError as e:
        return ("error", e.code)


def _setup_1d(ctx, g):
    """hip.OK, hip.NOTHING_TO_DO, or the library's error code (a graph without paths has no learning rate to start from)."""
    kind, rc = _outcome(lambda: ctx.setup_1d(_ygs(g), hip.make_config(**ONE_STREAM)))
    return rc


def _same_index(item, solo, where):
    """Item and solo context hold the same bits — and, now that both are built by the same kernels, each is ALSO held to the
    host's restatement of their graph (index_ref.py: gfs_shared_node_layout and the numpy records), which shares no code with them."""
    assert np.array_equal(item.node_layout(), solo.node_layout()), where
    got, want = item.step_records(), solo.step_records()
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), where
    assert not got[-1].any(), where                                    # the padding record
    host = HostIndex(solo.graph)
    host.check(item, f"{where}: item")
    host.check(solo, f"{where}: solo")


# ---- 1: a hostile mix -------------------------------------------------------------------------------------------------------------
def test_hostile_mix_items_equal_solo_contexts(mix):
    graphs, cset, solos = mix
    info = cset.info()
    assert (info.items, info.total_nodes, info.total_steps, info.total_paths) == \
        (len(graphs), sum(g.n_nodes for g in graphs), sum(g.n_steps for g in graphs), sum(g.n_paths for g in graphs))
    assert info.device_allocations == 3 and info.arena_bytes > 0 and info.build_ms > 0.0
    assert hip.lib().gfs_ctx_set_size(cset._h) == len(graphs) and hip.lib().gfs_ctx_set_item(cset._h, len(graphs)) is None
    rng = np.random.default_rng(17)
    for i, (g, item, solo) in enumerate(zip(graphs, cset.contexts, solos)):
        _same_index(item, solo, i)
        rc = _setup_1d(item, g)
        assert rc == _setup_1d(solo, g), i
        for ctx in (item, solo):
            if rc == hip.OK:
                ctx.init_positions()
        assert _outcome(item.download) == _outcome(solo.download), i
        if rc != hip.OK:
            continue
        x = rng.normal(size=g.n_nodes) * 100.0
        item.upload(x)
        solo.upload(x)
        got, want = item.pair_errors([1, 2, 7]), solo.pair_errors([1, 2, 7])
        assert got.tobytes() == want.tobytes(), i
    assert int(cset.contexts[10].pair_errors([1])["pairs"][0]) > 0      # (DRB1: the figures are of something)


# ---- 2: past one grid-stride pass of every kernel of the build --------------------------------------------------------------------
def _tiny(k):
    """Tiny graphs of many short paths: 56 paths each, so that 300 of them carry more paths than the paths kernel's grid."""
    rng = np.random.default_rng(100 + k)
    n = 2 + k
    paths = [list(rng.integers(0, n, int(rng.integers(0, 4)))) for _ in range(56)]
    return graph_from_paths(paths, rng.integers(1, 9, n + 1))           # (the last node is never visited)


def test_union_past_every_grid():
    drb1, tiny = load("DRB1-3123.gfa"), [_tiny(k) for k in range(3)]
    copies = 54
    # over steps (first_visit, node_stats, fill_records, the scan's input): 54 * 35059 steps > 2048 * 256
    assert copies * drb1.n_steps > STEP_PASS
    # over nodes (first_key, run_up, jump, anchor, branch_key, scatter): 54 * 4955 nodes > 1024 * 256
    assert copies * drb1.n_nodes > NODE_PASS
    # over paths and items (the paths kernel, which also zeroes the padding records): 300 * 56 + 54 * 12 paths + 354 items > 64 * 256
    assert 300 * 56 + copies * drb1.n_paths + 300 + copies > PATH_PASS
    graphs, kind = [], []
    for k in range(300):
        graphs.append(tiny[k % 3]); kind.append(k % 3)
        if k % 6 == 0 and kind.count(3) < copies:
            graphs.append(drb1); kind.append(3)
    while kind.count(3) < copies:
        graphs.append(drb1); kind.append(3)
    solos = [hip.Context(g) for g in tiny + [drb1]]
    want = [(c.node_layout(), c.step_records().tobytes()) for c in solos]
    hosts = [HostIndex(g) for g in tiny + [drb1]]                       # the host's restatement, once per distinct graph
    for k, (host, solo) in enumerate(zip(hosts, solos)):
        host.check(solo, f"solo {k}")
    cset = hip.ContextSet(graphs)
    try:
        info = cset.info()
        assert info.total_steps > STEP_PASS and info.total_nodes > NODE_PASS and info.total_paths + info.items > PATH_PASS
        for i, (item, k) in enumerate(zip(cset.contexts, kind)):
            assert np.array_equal(item.node_layout(), want[k][0]), (i, k)
            assert item.step_records().tobytes() == want[k][1], (i, k)
            assert np.array_equal(item.node_layout(), hosts[k].layout), (i, k)
            assert item.step_records().tobytes() == hosts[k].records.tobytes(), (i, k)
    finally:
        cset.close()
        for c in solos:
            c.close()


# ---- 3: runs ------------------------------------------------------------------------------------------------------------------------
def test_sort_and_layout_runs_equal_solo_runs(mix):
    graphs, cset, solos = mix
    ran = moved = 0
    for i, (g, item, solo) in enumerate(zip(graphs, cset.contexts, solos)):
        p2 = _layout_params(g)
        for ctx in (item, solo):
            ctx.rc1 = _setup_1d(ctx, g)
            if ctx.rc1 == hip.OK:
                ctx.init_positions()
                assert ctx.run() == hip.OK
                ctx.x1 = ctx.download()
        assert item.rc1 == solo.rc1, i
        if item.rc1 != hip.OK:
            continue
        assert item.x1.tobytes() == solo.x1.tobytes(), i
        moved += not np.array_equal(item.x1, hip.init_positions(g))      # (a linear graph starts where it ends)
        c0 = gaussian_init(g, 2, 9)
        for ctx in (item, solo):                                       # the layout reads path_len and the record after a step
            assert ctx.setup_nd(p2, hip.make_config(**ONE_STREAM)) == hip.OK
            ctx.upload(c0)
            assert ctx.run() == hip.OK
            ctx.x2 = ctx.download()
        assert item.x2.tobytes() == solo.x2.tobytes(), i
        assert not np.array_equal(item.x2, c0), i
        ran += 1
    assert ran >= 9 and moved >= 5


def test_batch_over_set_items_equals_batch_over_solo_contexts(mix):
    graphs, cset, solos = mix
    results = []
    for ctxs in (cset.contexts, solos):
        members = []
        for g, ctx in zip(graphs, ctxs):
            if _setup_1d(ctx, g) == hip.OK and ctx.stats().bundle == 1:
                members.append(ctx)
        b = hip.Batch(members)
        try:
            b.init_positions()
            b.run()
            xs, orders, _ = b.results()
            results.append(([x.tobytes() for x in xs], [o.tobytes() for o in orders], b.stats().items_run))
        finally:
            b.close()
    assert results[0] == results[1] and results[0][2] >= 9


# ---- 4: an error found on the device --------------------------------------------------------------------------------------------
def test_out_of_range_step_names_the_lowest_item_and_frees_everything():
    base = [load("lil.gfa"), load("simple.gfa"), absent_node_graph(), self_loop_graph(), load("lil.gfa"), load("simple.gfa"),
            load("DRB1-3123.gfa")]
    hip.ContextSet(base).close()                                        # (modules loaded, the runtime's pools warm)
    for i in (2, 5):
        bad = np.array(base[i].step_node, dtype=np.uint32)
        bad[len(bad) // 2] = base[i].n_nodes                            # one past the item's last node: a node of the NEXT item in the union
        base[i] = G.FlatGraph(node_len=base[i].node_len, step_node=bad, step_is_rev=base[i].step_is_rev,
                              path_first_step=base[i].path_first_step, node_ids=base[i].node_ids, path_names=base[i].path_names)
    # three samples around two failing creates: before, between, after.  A create that kept anything would lower both later ones.
    free = [_free_bytes()]
    for _ in range(2):
        with pytest.raises(hip.GfsError) as ei:
            hip.ContextSet(base)
        assert ei.value.code == E_ARG and "set item 2: " in str(ei.value) and "step_node out of range" in str(ei.value)
        del ei                                                          # (the traceback holds the frame of the failed create)
        free.append(_free_bytes())
    print("free device memory before, after one and after two failing creates:", free)
    assert free[1] == free[0] and free[2] == free[0]


# ---- 5: ownership -----------------------------------------------------------------------------------------------------------------
def test_destroy_on_an_item_is_ignored_and_setups_repeat():
    g = load("DRB1-3123.gfa")
    cset = hip.ContextSet([load("lil.gfa"), g])
    solo = hip.Context(g)
    try:
        item = cset.contexts[1]
        hip.lib().gfs_ctx_destroy(item._h)                              # the set's, not the caller's: nothing happens
        hip.lib().gfs_ctx_destroy(item._h)
        for ctx in (item, solo):
            assert ctx.setup_1d(_ygs(g), hip.make_config(**ONE_STREAM)) == hip.OK
            ctx.init_positions()
            assert ctx.run() == hip.OK
        assert item.download().tobytes() == solo.download().tobytes()
        c0 = gaussian_init(g, 3, 4)
        for ctx in (item, solo):                                       # again, with another shape
            assert ctx.setup_nd(_layout_params(g, dims=3), hip.make_config(n_streams=1000)) == hip.OK
            assert ctx.positions_len() == g.n_nodes * 6
            ctx.upload(c0)
        assert item.download().tobytes() == solo.download().tobytes()
        _same_index(item, solo, "after two setups")
    finally:
        solo.close()
        cset.close()


def test_twenty_set_cycles_leave_free_memory_where_it_was():
    graphs = [load(name) for name in ("DRB1-3123.gfa", "lil.gfa", "simple.gfa")] * 4
    free = []
    for _ in range(20):
        cset = hip.ContextSet(graphs)
        try:
            for g, ctx in zip(graphs, cset.contexts):
                assert ctx.setup_1d(_ygs(g, iter_max=3), hip.make_config(**ONE_STREAM)) == hip.OK
                ctx.init_positions()
                assert ctx.run() == hip.OK
            assert int(cset.contexts[0].pair_errors([1])["pairs"][0]) > 0
        finally:
            cset.close()
        free.append(_free_bytes())
    drift = free[0] - free[-1]
    print(f"free device memory after cycle 1: {free[0]} B, after cycle 20: {free[-1]} B, drift {drift} B")
    assert drift == 0


# ---- 6: what a build launches and allocates does not depend on the number of items ------------------------------------------------
def test_launches_and_allocations_do_not_grow_with_the_items():
    pair = [load("DRB1-3123.gfa"), load("lil.gfa")]
    infos = []
    for n in (4, 64):
        cset = hip.ContextSet(pair * (n // 2))
        infos.append(cset.info())
        cset.close()
    print("launches", infos[0].launches, infos[1].launches, "allocations", infos[0].device_allocations, infos[1].device_allocations,
          "build ms", infos[0].build_ms, infos[1].build_ms)
    assert infos[0].items == 4 and infos[1].items == 64
    assert infos[0].launches == infos[1].launches > 0
    assert infos[0].device_allocations == infos[1].device_allocations == 3


# ---- 7: the Python batch driver -----------------------------------------------------------------------------------------------------
def test_sort_batch_driver_builds_small_graphs_in_one_set(monkeypatch):
    graphs = [load("DRB1-3123.gfa"), load("simple.gfa"), G.synth_chain(20000, 3), load("lil.gfa")]
    params = [_ygs(g) for g in graphs]
    cfg = hip.make_config(**ONE_STREAM)
    seen = []
    real = hip.ContextSet

    def spy(gs, device=0):
        gs = list(gs)
        seen.append(gs)
        return real(gs, device=device)
    monkeypatch.setattr(hip, "ContextSet", spy)
    out, bs = S.path_sgd_sort_batch(graphs, params, cfg=cfg)
    assert len(seen) == 1 and [g is h for g, h in zip(seen[0], [graphs[0], graphs[1], graphs[3]])] == [True] * 3 and len(seen[0]) == 3
    for i, (g, p, res) in enumerate(zip(graphs, params, out)):
        x = S.path_linear_sgd(g, p, cfg=cfg)
        assert res["positions"].tobytes() == x.tobytes(), i
        assert np.array_equal(res["order"], S.path_sgd_sort(g, p, cfg=cfg)), i
    assert [r["batched"] for r in out] == [True, True, out[2]["batched"], True]
