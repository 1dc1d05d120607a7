"""Set setup on the device (gfs_ctx_set_setup_*, csrc/capi_set.hip; K3c in csrc/set_setup_kernels.hip): every item of a set, set up
in one pass, holds byte for byte what gfs_ctx_setup_1d / _nd leaves in a context of the same graph set up alone — RNG words, zeta
table, schedule table, counters, positions, team state and trace buffers — runs to the same bits, and owns nothing: the arrays
are the set's.  Integer arithmetic and host tables only, so there is no tolerance anywhere in this file."""
import copy

import numpy as np
import pytest

from util import G, P, load, graph_from_paths, gaussian_init, hub_graph
from index_ref import free_device_bytes as _free_bytes
from set_setup_ref import seeded_words, all_states, COUNTER_BYTES, ITER_CONSTS_BYTES
from test_gpu_multi_merge import Dev, _sync
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -5
ONE_STREAM = dict(n_streams=1)
PARENT_DRIFT_BYTES = 0                               # tests/test_gpu_ownership.py: free device memory does not drift


def _chain(n, seed=1):
    rng = np.random.default_rng(seed)
    return graph_from_paths([list(range(n)), list(range(n // 3, n))], rng.integers(1, 9, n))


def _base_1d(iter_max=6, updates=2000):
    p = P.YgsParams.from_graph(load("lil.gfa"), 0, 1).path_sgd
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _base_nd(dims, iter_max=5, updates=2000):
    p = P.LayoutSGDParams.from_graph(load("lil.gfa"), dims, 1)
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _with(p, **kw):
    q = copy.copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _mix():
    """(graph, seed, launch config) per item: the fixtures, a graph of 0 nodes, a graph whose paths all have one step BETWEEN two
    ordinary items, chains forced to 255, 256 and 257 streams (either side of the seeding kernel's workgroup), a one-stream item;
    every item its own seed, one of them 2^64 - 2 (seed + t wraps inside the item), one with a stream base."""
    return [
        (load("simple.gfa"), 11, None),
        (load("lil.gfa"), (1 << 64) - 2, hip.make_config(n_streams=70)),
        (load("DRB1-3123.gfa"), 9399220, None),
        (graph_from_paths([], []), 5, None),
        (_chain(300, 2), 17, hip.make_config(n_streams=255)),
        (graph_from_paths([[0], [2], [1]], [3, 4, 5]), 23, None),
        (_chain(400, 3), 29, hip.make_config(n_streams=256, stream_base=(1 << 64) - 100)),
        (_chain(500, 4), 31, hip.make_config(n_streams=257, stream_base=7)),
        (load("lil.gfa"), 0, hip.make_config(**ONE_STREAM)),
    ]


def _facts(ctx, rc):
    """The host side of a setup, as far as the ABI shows it."""
    st = ctx.stats()
    return (rc, ctx.positions_len(), int(st.n_streams), int(st.bundle), int(st.run_trips), ctx.kshift() if rc == hip.OK else None)


def _same_as_solo(item, rc, g, setup, where):
    """The item against a second context of the same graph set up alone; returns the solo context's state arrays."""
    solo = hip.Context(g)
    try:
        solo_rc = setup(solo)
        assert rc == solo_rc, where
        assert _facts(item, rc) == _facts(solo, solo_rc), where
        got, want = all_states(item), all_states(solo)
        for kind in range(hip.STATE_KINDS):
            assert len(got[kind]) == len(want[kind]), (where, kind)
            assert got[kind] == want[kind], (where, kind)
        return want
    finally:
        solo.close()


# ---- 1: state, byte for byte -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2, 3, 8])
def test_every_state_array_equals_the_single_setups(dims):
    mix = _mix()
    graphs = [g for g, _, _ in mix]
    base = _base_1d() if dims == 0 else _base_nd(dims)
    params = [_with(base, seed=seed) for _, seed, _ in mix]
    cfgs = [cfg for _, _, cfg in mix]
    cset = hip.ContextSet(graphs)
    try:
        rcs = cset.setup_1d(params, cfgs) if dims == 0 else cset.setup_nd(params, cfgs)
        assert rcs == [hip.OK, hip.OK, hip.OK, hip.NOTHING_TO_DO, hip.OK, hip.NOTHING_TO_DO, hip.OK, hip.OK, hip.OK]
        info = cset.setup_info
        assert (info.items, info.configured, info.nothing_to_do) == (9, 7, 2)
        streams = 0
        for i, (g, seed, cfg) in enumerate(mix):
            item = cset.contexts[i]
            setup = (lambda c: c.setup_1d(params[i], cfg)) if dims == 0 else (lambda c: c.setup_nd(params[i], cfg))
            want = _same_as_solo(item, rcs[i], g, setup, f"dims {dims} item {i}")
            x_len = g.n_nodes * (2 * dims if dims else 1)
            assert len(want[hip.STATE_POSITIONS]) == 8 * x_len and not any(want[hip.STATE_POSITIONS])
            if rcs[i] != hip.OK:                                        # nothing but the zeroed replica (none for 0 nodes)
                assert all(len(want[k]) == 0 for k in range(1, hip.STATE_KINDS)), i
                continue
            T = int(item.stats().n_streams)
            streams += T
            if cfg is not None:
                assert T == cfg.n_streams, i
            rng = item.debug_sgd_state(hip.STATE_RNG)
            assert np.array_equal(rng, seeded_words(seed, cfg.stream_base if cfg is not None else 0, T)), i
            assert len(want[hip.STATE_COUNTERS]) == COUNTER_BYTES and not any(want[hip.STATE_COUNTERS])
            assert len(want[hip.STATE_SCHEDULE]) == ITER_CONSTS_BYTES * (base.iter_max + 1)
            zetas = item.debug_sgd_state(hip.STATE_ZETAS)
            assert zetas[0] == 0.0 and zetas[1] > 0.0                   # (a table, not zeros)
        assert info.total_streams == streams
        assert (info.device_allocations, info.copies, info.launches) == (2, 1, 2) and info.state_bytes > 0 and info.setup_ms > 0.0
    finally:
        cset.close()


# ---- 2: runs -----------------------------------------------------------------------------------------------------------------------
def _run_graphs():
    return [load("simple.gfa"), load("lil.gfa"), load("DRB1-3123.gfa"), hub_graph(900, 4)]


def test_batch_of_a_set_setup_runs_to_the_solo_bits_1d():
    graphs = _run_graphs()
    params = [_with(_base_1d(iter_max=4, updates=1500), seed=100 + i) for i in range(len(graphs))]
    cfg = hip.make_config(**ONE_STREAM)
    want = []
    for g, p in zip(graphs, params):
        ctx = hip.Context(g)
        try:
            assert ctx.setup_1d(p, cfg) == hip.OK
            ctx.init_positions()
            assert ctx.run() == hip.OK
            want.append(ctx.download())
        finally:
            ctx.close()
    cset = hip.ContextSet(graphs)
    batch = None
    try:
        assert cset.setup_1d(params, cfg) == [hip.OK] * len(graphs)
        batch = hip.Batch(cset.contexts)
        batch.init_positions()
        assert batch.run() == hip.OK
        xs, _, _ = batch.results()
        for i, g in enumerate(graphs):
            assert xs[i].tobytes() == want[i].tobytes(), i
            assert not np.array_equal(want[i], hip.init_positions(g)), i
    finally:
        if batch is not None:
            batch.close()
        cset.close()


def test_batch_of_a_set_setup_runs_to_the_solo_bits_2d():
    graphs = _run_graphs()
    params = [_with(_base_nd(2, iter_max=4, updates=1500), seed=200 + i) for i in range(len(graphs))]
    starts = [gaussian_init(g, 2, 7 + i) for i, g in enumerate(graphs)]
    cfg = hip.make_config(**ONE_STREAM)
    want = []
    for g, p, c0 in zip(graphs, params, starts):
        ctx = hip.Context(g)
        try:
            assert ctx.setup_nd(p, cfg) == hip.OK
            ctx.upload(c0)
            assert ctx.run() == hip.OK
            want.append(ctx.download())
        finally:
            ctx.close()
    cset = hip.ContextSet(graphs)
    batch = None
    try:
        assert cset.setup_nd(params, cfg) == [hip.OK] * len(graphs)
        batch = hip.Batch(cset.contexts)
        batch.upload_coords(starts)
        assert batch.run() == hip.OK
        coords, _ = batch.coords()
        for i in range(len(graphs)):
            assert coords[i].tobytes() == want[i].tobytes(), i
            assert not np.array_equal(want[i], starts[i]), i
    finally:
        if batch is not None:
            batch.close()
        cset.close()


def test_an_item_of_a_4d_set_runs_alone_to_the_solo_bits():
    graphs = [load("simple.gfa"), load("lil.gfa"), hub_graph(900, 4)]
    params = [_with(_base_nd(4, iter_max=4, updates=1500), seed=300 + i) for i in range(len(graphs))]
    cfg = hip.make_config(**ONE_STREAM)
    c0 = gaussian_init(graphs[2], 4, 9)
    solo = hip.Context(graphs[2])
    cset = hip.ContextSet(graphs)
    try:
        assert solo.setup_nd(params[2], cfg) == hip.OK
        solo.upload(c0)
        assert solo.run() == hip.OK
        assert cset.setup_nd(params, cfg) == [hip.OK] * 3
        before = [all_states(c) for c in cset.contexts[:2]]
        item = cset.contexts[2]
        item.upload(c0)
        assert item.run() == hip.OK
        got = item.download()
        assert got.tobytes() == solo.download().tobytes() and not np.array_equal(got, c0)
        assert int(item.stats().term_updates) == int(solo.stats().term_updates) == 5 * 1500
        assert [all_states(c) for c in cset.contexts[:2]] == before      # the neighbours in the arena are untouched
    finally:
        solo.close()
        cset.close()


# ---- 3: other shapes ---------------------------------------------------------------------------------------------------------------
def test_team_kernel_and_tracing_items_get_the_single_setups_shape_and_zero_state():
    """A team-kernel item (bundles of 64 on a chain of 20 000 nodes) and a tracing item beside an ordinary one: the same shape
    and plan as set up alone, the same zeroed team state and trace buffers.  Nothing runs full-width here: those runs race."""
    graphs = [_chain(20000, 6), load("lil.gfa"), load("DRB1-3123.gfa")]
    params = [_with(_base_1d(), seed=400 + i) for i in range(3)]
    cfgs = [hip.make_config(flags=hip.F_BUNDLE(64)), hip.make_config(n_streams=3, trace_per_stream=1), None]
    cset = hip.ContextSet(graphs)
    try:
        rcs = cset.setup_1d(params, cfgs)
        assert rcs == [hip.OK] * 3
        for i, g in enumerate(graphs):
            want = _same_as_solo(cset.contexts[i], rcs[i], g, lambda c: c.setup_1d(params[i], cfgs[i]), f"item {i}")
            T = int(cset.contexts[i].stats().n_streams)
            if i == 0:
                assert int(cset.contexts[0].stats().bundle) == 64 and T % 64 == 0
                assert len(want[hip.STATE_LEAD]) == 8 * T * 4 and not any(want[hip.STATE_LEAD])
            else:
                assert len(want[hip.STATE_LEAD]) == 0
            if i == 1:
                assert len(want[hip.STATE_TRACE]) == 3 * 16 and not any(want[hip.STATE_TRACE])
                assert len(want[hip.STATE_TRACE_COUNTS]) == 3 * 4 and not any(want[hip.STATE_TRACE_COUNTS])
            else:
                assert len(want[hip.STATE_TRACE]) == 0 and len(want[hip.STATE_TRACE_COUNTS]) == 0
        info = cset.setup_info
        assert (info.device_allocations, info.copies, info.launches) == (2, 1, 2)
    finally:
        cset.close()


# ---- 4: ownership ------------------------------------------------------------------------------------------------------------------
def _sorted_alone(g, p):
    ctx = hip.Context(g)
    try:
        assert ctx.setup_1d(p, hip.make_config(**ONE_STREAM)) == hip.OK
        ctx.init_positions()
        assert ctx.run() == hip.OK
        return ctx.download()
    finally:
        ctx.close()


def test_set_setup_again_1d_2d_1d():
    graphs = _run_graphs()
    p1 = [_with(_base_1d(iter_max=3, updates=1000), seed=500 + i) for i in range(len(graphs))]
    p2 = [_with(_base_nd(2, iter_max=3, updates=1000), seed=600 + i) for i in range(len(graphs))]
    cfg = hip.make_config(**ONE_STREAM)
    cset = hip.ContextSet(graphs)
    try:
        out, allocations = [], []
        for dims in (0, 2, 0):
            assert (cset.setup_1d(p1, cfg) if dims == 0 else cset.setup_nd(p2, cfg)) == [hip.OK] * len(graphs)
            allocations.append(int(cset.setup_info.device_allocations))
            run = []
            for i, (ctx, g) in enumerate(zip(cset.contexts, graphs)):
                assert ctx.positions_len() == g.n_nodes * (2 * dims if dims else 1)
                if dims == 0:
                    ctx.init_positions()
                else:
                    ctx.upload(gaussian_init(g, 2, 40 + i))
                assert ctx.run() == hip.OK
                run.append(ctx.download())
            out.append(run)
        # arena and staging; the arena grown for the layouts' fourfold positions (the staged tables need not be larger); both reused
        assert allocations[0] == 2 and allocations[1] in (1, 2) and allocations[2] == 0
        for i, g in enumerate(graphs):
            assert out[2][i].tobytes() == out[0][i].tobytes(), i
            assert out[0][i].tobytes() == _sorted_alone(g, p1[i]).tobytes(), i
            assert np.isfinite(out[1][i]).all()
    finally:
        cset.close()


def test_a_single_setup_of_one_item_leaves_the_neighbours_in_the_arena():
    graphs = _run_graphs()
    params = [_with(_base_1d(iter_max=3, updates=1000), seed=700 + i) for i in range(len(graphs))]
    cfg = hip.make_config(**ONE_STREAM)
    cset = hip.ContextSet(graphs)
    try:
        assert cset.setup_1d(params, cfg) == [hip.OK] * len(graphs)
        before = [all_states(c) for c in cset.contexts]
        mid = cset.contexts[1]
        other = _with(params[1], seed=999, iter_max=5)
        assert mid.setup_1d(other, hip.make_config(n_streams=2)) == hip.OK    # arrays of its own from here on
        assert len(mid.debug_sgd_state(hip.STATE_RNG)) == 8 and np.array_equal(mid.debug_sgd_state(hip.STATE_RNG), seeded_words(999, 0, 2))
        mid.init_positions()
        assert mid.run() == hip.OK
        assert int(mid.stats().term_updates) == 6 * 1000
        for i in (0, 2, 3):
            assert all_states(cset.contexts[i]) == before[i], i
        for i in (0, 2, 3):                                             # ... and they still run to the solo bits
            cset.contexts[i].init_positions()
            assert cset.contexts[i].run() == hip.OK
            assert cset.contexts[i].download().tobytes() == _sorted_alone(graphs[i], params[i]).tobytes(), i
        # a second set setup takes the item back into the arena
        assert cset.setup_1d(params, cfg) == [hip.OK] * len(graphs)
        assert [all_states(c) for c in cset.contexts] == before
    finally:
        cset.close()


def test_a_bound_position_buffer_on_an_item_stays_the_callers():
    graphs = _run_graphs()
    params = [_with(_base_1d(iter_max=3, updates=1000), seed=800 + i) for i in range(len(graphs))]
    cfg = hip.make_config(**ONE_STREAM)
    cset = hip.ContextSet(graphs)
    ext = None
    try:
        assert cset.setup_1d(params, cfg) == [hip.OK] * len(graphs)
        item, g = cset.contexts[2], graphs[2]
        own = item.positions_device()
        ext = Dev(g.n_nodes, np.float64)
        ext.set(hip.init_positions(g)[np.argsort(item.node_layout())])  # device order: slot perm[k] holds node k
        item.bind_positions(ext.ptr)
        assert item.positions_device() == ext.ptr != own
        assert item.run() == hip.OK
        got = item.download()
        assert got.tobytes() == _sorted_alone(g, params[2]).tobytes()
        held = ext.host()
        assert got.tobytes() == held[item.node_layout()].tobytes()
        assert cset.setup_1d(params, cfg) == [hip.OK] * len(graphs)      # lets go of the bound vector: back into the arena
        assert item.positions_device() != ext.ptr
        cset.close()
        _sync()
        assert ext.host().tobytes() == held.tobytes()                   # the caller's, still there once the set has gone
    finally:
        cset.close()
        if ext is not None:
            ext.free()


def test_twenty_create_setup_destroy_rounds_leave_free_memory_where_it_was():
    graphs = [load("simple.gfa"), load("lil.gfa"), load("DRB1-3123.gfa"), _chain(20000, 6)]
    params = [_with(_base_1d(iter_max=3, updates=1000), seed=i) for i in range(4)]
    cfgs = [None, hip.make_config(n_streams=5, trace_per_stream=2), None, hip.make_config(flags=hip.F_BUNDLE(64))]
    free = []
    for _ in range(20):
        cset = hip.ContextSet(graphs)
        try:
            assert cset.setup_1d(params, cfgs) == [hip.OK] * 4
            assert cset.contexts[1].setup_1d(params[1]) == hip.OK       # one item with arrays of its own when the set goes
        finally:
            cset.close()
        free.append(_free_bytes())
    drift = free[0] - free[-1]
    print(f"free device memory after round 1: {free[0]} B, after round 20: {free[-1]} B, drift {drift} B")
    assert drift <= PARENT_DRIFT_BYTES


def test_a_refused_item_is_named_and_every_item_is_left_as_it_was():
    graphs = _run_graphs() + [load("lil.gfa")]
    params = [_with(_base_1d(iter_max=3, updates=1000), seed=900 + i) for i in range(5)]
    cfg = hip.make_config(**ONE_STREAM)
    cset = hip.ContextSet(graphs)
    try:
        assert cset.setup_1d(params, cfg) == [hip.OK] * 5
        before = [all_states(c) for c in cset.contexts]
        info = cset.setup_info
        bad = list(params)
        bad[2] = _with(params[2], theta=1.0)                            # check_setup_args: theta must be in [0,1)
        bad[4] = _with(params[4], eta_max=0.0)                          # ... and a later one: the lowest is named
        with pytest.raises(hip.GfsError) as ei:
            cset.setup_1d(bad, cfg)
        assert ei.value.code == E_ARG and "set item 2: theta must be in [0,1)" in str(ei.value)
        nd = [_with(_base_nd(2), seed=i) for i in range(5)]
        nd[3] = _with(nd[3], dimensions=9)
        nd[4] = _with(nd[4], theta=-0.5)
        with pytest.raises(hip.GfsError) as ei:
            cset.setup_nd(nd, cfg)
        assert ei.value.code == E_UNSUPPORTED and "set item 3: dimensions must be 1..8" in str(ei.value)
        shape = [cfg] * 5
        shape[1] = hip.make_config(n_streams=1, block_size=100)         # refused by the launch policy, after the arguments
        with pytest.raises(hip.GfsError) as ei:
            cset.setup_1d(params, shape)
        assert ei.value.code == E_ARG and "set item 1: block_size must be a multiple of 64" in str(ei.value)
        assert [all_states(c) for c in cset.contexts] == before
        after = cset.setup_info
        assert (after.items, after.configured, after.total_streams, after.state_bytes) == (info.items, info.configured, info.total_streams, info.state_bytes)
        for i in (0, 2, 4):                                             # still set up, and still the solo bits
            cset.contexts[i].init_positions()
            assert cset.contexts[i].run() == hip.OK
            assert cset.contexts[i].download().tobytes() == _sorted_alone(graphs[i], params[i]).tobytes(), i
    finally:
        cset.close()


# ---- 5: what a set setup allocates, copies and launches does not depend on the number of items -----------------------------------------
def test_allocations_copies_and_launches_do_not_grow_with_the_items():
    g = load("DRB1-3123.gfa")
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    counts = []
    for n in (3, 64):
        cset = hip.ContextSet([g] * n)
        try:
            assert cset.setup_1d([_with(p, seed=i) for i in range(n)]) == [hip.OK] * n
            info = cset.setup_info
            T = int(cset.contexts[0].stats().n_streams)
            assert info.items == info.configured == n and info.total_streams == n * T
            assert np.array_equal(cset.contexts[n - 1].debug_sgd_state(hip.STATE_RNG), seeded_words(n - 1, 0, T))
            counts.append((int(info.device_allocations), int(info.copies), int(info.launches)))
        finally:
            cset.close()
    print("set setup of 3 and of 64 DRB1 items: (allocations, copies, launches) =", counts)
    assert counts[0] == counts[1] == (2, 1, 2)
