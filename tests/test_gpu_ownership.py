"""Who owns what on the device (csrc/device_memory.h: gfs::Buffer, its borrowed state, gfs::EventPair), at the switches of
ownership that no feature test walks through: a position vector the caller binds, a context set up again and again with another
shape, a create that fails half way, a rank that trades its own exchange buffer for the caller's, and many contexts created and
destroyed in a row.  Results are compared bit for bit at one reference stream (what tests/test_gpu_parity.py holds equal to the
oracle); the caller's buffers come from the HIP runtime the library is linked to, as in tests/test_gpu_multi_merge.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import multi_cases as MC
from test_gpu_multi_merge import Dev, _rt, _sync
from util import G, P, hub_graph, reverse_short_paths_graph, gaussian_init
from gfasort_amd import hip
from gfasort_amd.distributed import SHARDING

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
ONE_STREAM = dict(n_streams=1)


def _ygs(g, iter_max=4, updates=3000):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _layout_params(g, dims=2, iter_max=3, updates=2000):
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max, p.min_term_updates = iter_max, updates
    return p


def _sorted_fresh(g, p, x0):
    """The whole schedule on a fresh context that owns its positions."""
    ctx = hip.Context(g)
    try:
        assert ctx.setup_1d(p, hip.make_config(**ONE_STREAM)) == hip.OK
        ctx.upload(x0)
        assert ctx.run() == hip.OK
        return ctx.download()
    finally:
        ctx.close()


# ---- 1: a bound position vector is the caller's ------------------------------------------------------------------------------
def test_bound_positions_stay_the_callers():
    g = hub_graph()
    p = _ygs(g)
    x0 = hip.init_positions(g)
    want = _sorted_fresh(g, p, x0)
    assert not np.array_equal(want, x0)
    ctx = hip.Context(g)
    ext = None
    try:
        assert ctx.setup_1d(p, hip.make_config(**ONE_STREAM)) == hip.OK
        n = ctx.positions_len()
        assert n == g.n_nodes
        ext = Dev(n, np.float64)
        ext.set(x0[np.argsort(ctx.node_layout())])                      # device order: slot perm[k] holds node k
        ctx.bind_positions(ext.ptr)
        assert ctx.positions_device() == ext.ptr
        assert ctx.run() == hip.OK
        got = ctx.download()
        held = ext.host()
        assert got.tobytes() == held[ctx.node_layout()].tobytes()       # what the context reads is what the caller holds
        assert got.tobytes() == want.tobytes()
        assert ctx.setup_1d(p, hip.make_config(**ONE_STREAM)) == hip.OK  # lets go of the bound vector, allocates its own
        assert ctx.positions_device() != ext.ptr
        ctx.close()
        _sync()
        assert ext.host().tobytes() == held.tobytes()
        ext.set(np.full(n, 7.5))
        assert np.array_equal(ext.host(), np.full(n, 7.5))
    finally:
        ctx.close()
        if ext is not None:
            ext.free()


# ---- 2: one context, three setups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trace", [0, 8])
def test_setup_again_1d_2d_1d(trace):
    g = hub_graph()
    p1, p2 = _ygs(g), _layout_params(g)
    x0 = hip.init_positions(g)
    c0 = gaussian_init(g, 2, 5)
    ctx = hip.Context(g)
    try:
        out = []
        for dims in (0, 2, 0):
            if dims == 0:
                assert ctx.setup_1d(p1, hip.make_config(**ONE_STREAM)) == hip.OK
                assert ctx.positions_len() == g.n_nodes
                ctx.upload(x0)
            else:
                assert ctx.setup_nd(p2, hip.make_config(trace_per_stream=trace, **ONE_STREAM)) == hip.OK
                assert ctx.positions_len() == g.n_nodes * 2 * dims
                ctx.upload(c0)
            assert ctx.run() == hip.OK
            out.append(ctx.download())
            if dims and trace:
                tr, counts = ctx.trace()
                assert tr.shape == (1, trace) and int(counts[0]) > 0
        assert np.isfinite(out[1]).all() and not np.array_equal(out[1], c0)
        assert not np.array_equal(out[0], x0)
        assert out[2].tobytes() == out[0].tobytes()
        term, count = np.zeros(1, dtype=hip.TERM_DTYPE), np.zeros(1, dtype=np.uint64)
        with pytest.raises(hip.GfsError) as e:                          # the last setup asked for no trace: the second's is gone
            hip.check(hip.lib().gfs_ctx_trace(ctx._h, hip._ptr(term), 1, hip._ptr(count), 1))
        assert e.value.code == E_STATE
    finally:
        ctx.close()


# ---- 3: a failed create leaves a working process -------------------------------------------------------------------------------
def test_failed_creates_then_a_healthy_one():
    g = reverse_short_paths_graph()
    p = _ygs(g)
    x0 = hip.init_positions(g) + np.random.default_rng(3).normal(0.0, 30.0, g.n_nodes)   # (the start itself has no error to move)
    before = _sorted_fresh(g, p, x0)
    identity = np.arange(g.n_nodes, dtype=np.uint32)
    twice = identity.copy()
    twice[5] = twice[4]
    bad = copy.copy(g)
    bad.step_node = g.step_node.copy()
    bad.step_node[g.n_steps // 2] = g.n_nodes                          # one past the last node, in the middle of a path
    for graph, perm in ((g, twice), (bad, None), (bad, identity)):
        with pytest.raises(hip.GfsError) as e:
            hip.Context(graph, node_perm=perm)
        assert e.value.code == E_ARG
    assert _sorted_fresh(g, p, x0).tobytes() == before.tobytes()
    assert not np.array_equal(before, x0)


# ---- 4: a rank's exchange buffer, its own and then the caller's -----------------------------------------------------------------
def _one_window(case, own_first):
    """Two ranks in this process, one window and its merge.  own_first: every rank first allocates its exchange buffer, then
    is bound to the caller's.  Returns each rank's positions and what the caller's buffers held after the ranks were destroyed."""
    g, p = MC.graph(case.graph), MC.params(case)
    ranks = [hip.Rank(g, p, case.dims, r, case.world, device=0, sharding=SHARDING[case.sharding], merge_every=case.merge_every,
                      merge_rule=case.merge, payload_f64=case.f64, launch=hip.make_config(**ONE_STREAM)) for r in range(case.world)]
    bufs = []
    try:
        count = ranks[0].exchange_count()
        assert count > 0
        for rk in ranks:
            if own_first:
                own = hip.lib().gfs_rank_exchange_buffer(rk._h)
                assert own and hip.lib().gfs_rank_exchange_buffer(rk._h) == own
            bufs.append(Dev(count, np.float32))
            rk.bind_exchange_buffer(bufs[-1].ptr)
            assert hip.lib().gfs_rank_exchange_buffer(rk._h) == bufs[-1].ptr
            rk.set_positions(None)
        for rk in ranks:
            rk.window_begin([0, 1, 2])
        _sync()
        s = bufs[0].host() + bufs[1].host()
        assert np.any(s != 0)
        for b in bufs:
            b.set(s)
        for rk in ranks:
            rk.window_end()
        xs = [rk.get_positions() for rk in ranks]
        _sync()
        for rk in ranks:
            rk.close()
        after = [b.host() for b in bufs]                                # the caller's, still there once the ranks are gone
        assert all(a.tobytes() == s.tobytes() for a in after)
        return xs
    finally:
        for rk in ranks:
            rk.close()
        for b in bufs:
            b.free()


def test_rank_trades_its_exchange_buffer_for_the_callers():
    case = MC.BY_ID["A-w2-anneal-f32-e1"]
    assert case.world == 2 and case.dims == 0 and not case.f64
    want = _one_window(case, own_first=False)
    got = _one_window(case, own_first=True)
    for r in range(case.world):
        assert got[r].tobytes() == want[r].tobytes(), r
    assert not np.array_equal(want[0], hip.init_positions(MC.graph(case.graph)))


# ---- 5: no drift in free device memory ------------------------------------------------------------------------------------------
# Free bytes as hipMemGetInfo of the library's own runtime reports them (what torch.cuda.mem_get_info wraps; torch's copy of
# the runtime cannot be started in the suite's process, tests/test_gpu_multi_merge.py).  The bound is the drift of the library
# before device_memory.h on this same loop, profiles/r15/ownership.log.
PARENT_DRIFT_BYTES = 0


def _free_bytes():
    L = _rt()
    free, total = C.c_size_t(0), C.c_size_t(0)
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    _sync()
    assert L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def test_twenty_contexts_leave_free_memory_where_it_was():
    n = 200_000
    rng = np.random.default_rng(11)
    steps = np.concatenate([np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1]])
    g = G.FlatGraph(node_len=rng.integers(1, 9, n).astype(np.uint32), step_node=steps,
                    step_is_rev=(rng.random(2 * n) < 0.3).astype(np.uint8), path_first_step=np.array([0, n, 2 * n], dtype=np.uint64),
                    node_ids=np.arange(1, n + 1, dtype=np.uint64), path_names=["a", "b"])
    p = _ygs(g, iter_max=3, updates=100_000)
    free = []
    for _ in range(20):
        ctx = hip.Context(g)
        try:
            assert ctx.setup_1d(p) == hip.OK
            ctx.init_positions()
            ctx.run_range([0, 1])
            ctx.synchronize()
            assert int(ctx.pair_errors([1])["pairs"][0]) > 0
        finally:
            ctx.close()
        free.append(_free_bytes())
    drift = free[0] - free[-1]
    print(f"free device memory after cycle 1: {free[0]} B, after cycle 20: {free[-1]} B, drift {drift} B")
    assert drift <= PARENT_DRIFT_BYTES
