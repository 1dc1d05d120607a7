"""The 8-byte trip records of the 1D team kernels at B = 64 (sgd_1d.h TripRec, launch_policy.h compact_records).

T1  one wave with trip records == the same wave with GFS_F_FULL_RECORDS, bit for bit, fused and per-iteration, on a graph where
    twin, fused and generic trips all run.
T2  a path that passes 2^32 bp keeps 16-byte records and equals the mirror; the limit itself: 2^32 - 1 is eligible, 2^32 is not.
T3  crowded graphs (a hub, tandem repeats) keep 16-byte records; the record width follows the crowding onset.
T4  many waves on a small full-width window graph keep its exact chain order with trip records."""
import numpy as np
import pytest

from util import O, G, P, oracle_graph, oracle_params, graph_from_paths, hub_graph, np_crowding
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

B64 = hip.F_BUNDLE(64)


def _ygs(g, iter_max, mtu):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max, p.min_term_updates = iter_max, mtu
    p.space = min(p.space, 20_000)          # (the derived space is the longest path in bp: cap the zeta table)
    return p


def _node_slots(g):
    from gfasort_amd.distributed import path_order_layout
    return path_order_layout(g)


def _one_wave(g, p, flags):
    """One wave at B = 64 from the reference's start: (position bits, term_updates, attempts, launches, record bytes)."""
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64 | flags))
    width = ctx.record_bytes()
    ctx.upload(hip.init_positions(g))
    ctx.run()
    st = ctx.stats()
    x = ctx.download()
    ctx.close()
    return x.view(np.uint64), st.term_updates, st.attempts, st.launches, width


def _mirror(g, p, kshift):
    og = oracle_graph(g)
    st_o = O.State(og, oracle_params(p), n_streams=64, bundle=64, node_slots=_node_slots(g), chain=64, fused_trip=True, partners=2,
                   twin_trip=True, crowd_kshift=kshift)
    x = O.init_positions(og)
    st_o.run(x)
    so = st_o.stats()
    return x.view(np.uint64), so.term_updates, so.attempts


def mixed_graph(seed=21):
    """3000 nodes of 1..4 bp in a chain; paths of 2000, 1300, 1500 (every 4th node skipped: bubbles), 300 and 100 steps — the last
    one shorter than 2B = 128 steps, which lane 0 takes alone —, a fifth of the steps reverse.  No path visits a node twice."""
    rng = np.random.default_rng(seed)
    skipping = np.arange(1000, 3000)
    paths = [np.arange(0, 2000), np.arange(500, 1800), skipping[skipping % 4 != 1], np.arange(2500, 2800), np.arange(100, 200)]
    n_steps = sum(len(pth) for pth in paths)
    return graph_from_paths([pth.tolist() for pth in paths], rng.integers(1, 5, 3000), rev=rng.random(n_steps) < 0.2)


_T1 = {}


def _t1():
    """The graph, its parameters (21 iterations: first_cooling = 10 is crossed) and the full-record runs, made once."""
    if not _T1:
        g = mixed_graph()
        p = _ygs(g, 20, 20_000)
        _T1.update(g=g, p=p, full={extra: _one_wave(g, p, hip.F_FULL_RECORDS | extra) for extra in (0, hip.F_NO_FUSE)})
    return _T1["g"], _T1["p"], _T1["full"]


@pytest.mark.parametrize("extra", [0, hip.F_NO_FUSE], ids=["fused", "per-iteration"])
def test_trip_records_equal_step_records_bit_for_bit(extra):
    g, p, full = _t1()
    assert [int(c) for c in np.diff(g.path_first_step)] == [2000, 1300, 1500, 300, 100] and g.step_is_rev.any()
    _, _, a, b = np_crowding(g)
    assert b.max() == 0 and a.max() == 2                      # a node lies on at most 3 paths; nothing crowded at the onset below
    assert int(p.cooling_start * p.iter_max) == 10 and p.iter_max == 20
    x8, done8, att8, launches8, width8 = _one_wave(g, p, extra)
    x16, done16, att16, launches16, width16 = full[extra]
    assert (width8, width16) == (8, 16)
    assert launches8 == launches16 == (1 if extra == 0 else 21)
    assert done8 == done16 == 21 * 20_000 and att8 == att16
    assert np.array_equal(x8, x16)


def test_every_trip_form_ran():
    """The three trip forms of sgd_1d.h are all in the run of T1: without twin trips (GFS_F_DBG_NO_TWIN_TRIP: the partners as two
    generic trips, a's node takes two adds instead of their sum) and without fused trips (GFS_F_DBG_NO_FUSED_TRIP: two colours, two
    adds) the positions come out different, which they could not if no trip of that form had run; generic trips are what remains
    (the 100-step path has no other).  Each of those runs, too, is the same with both record widths."""
    g, p, full = _t1()
    x8, done8, att8, _, width8 = _one_wave(g, p, 0)
    assert width8 == 8
    for flag in (hip.F_DBG_NO_TWIN_TRIP, hip.F_DBG_NO_FUSED_TRIP, hip.F_DBG_NO_TWIN_TRIP | hip.F_DBG_NO_FUSED_TRIP):
        x, done, att, _, width = _one_wave(g, p, flag)
        assert width == 8 and done == done8
        assert not np.array_equal(x, x8), f"flags {flag:#x} change nothing: that trip form never ran"
        x16, done16, att16, _, width16 = _one_wave(g, p, flag | hip.F_FULL_RECORDS)
        assert width16 == 16 and (done16, att16) == (done, att) and np.array_equal(x16, x)


# ---- T2: the position limit --------------------------------------------------------------------------------------------
def long_node_graph(last_position):
    """One path of 1500 steps over a chain of 1500 nodes whose LAST step's position is last_position: nodes of 1..4 bp, and five
    very long ones at steps 700..704, in the middle of a run of 64 steps, that carry the rest."""
    rng = np.random.default_rng(33)
    n = 1500
    node_len = rng.integers(1, 5, n).astype(np.uint64)
    node_len[700:705] = 0
    rest = last_position - int(node_len[:n - 1].sum())
    assert rest > 5
    node_len[700:705] = rest // 5
    node_len[700] += rest % 5
    assert int(node_len[:n - 1].sum()) == last_position and node_len.max() < 1 << 32
    return graph_from_paths([list(range(n))], node_len.astype(np.uint32), rev=rng.random(n) < 0.2)


@pytest.mark.parametrize("last,width", [((1 << 32) - 1, 8), (1 << 32, 16), (5 << 30, 16)], ids=["2^32-1", "2^32", "5*2^30"])
def test_position_limit(last, width):
    g = long_node_graph(last)
    pos = np.concatenate([[0], np.cumsum(g.node_len.astype(np.uint64))[:-1]])
    assert int(pos.max()) == last and int(pos[699]) < 1 << 31     # the positions pass 2^32 (where they do) inside steps 700..705
    if last == 5 << 30:
        assert int(pos[704]) < 1 << 32 <= int(pos[705])
    p = _ygs(g, 6, 20_000)
    x, done, att, _, w = _one_wave(g, p, 0)
    assert w == width
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64))
    ks = ctx.kshift()
    ctx.close()
    xm, donem, attm = _mirror(g, p, ks)
    assert (done, att) == (donem, attm) and done == 7 * 20_000
    assert np.array_equal(x, xm)
    if width == 8:
        x16, done16, att16, _, w16 = _one_wave(g, p, hip.F_FULL_RECORDS)
        assert w16 == 16 and (done16, att16) == (done, att) and np.array_equal(x16, x)


# ---- T3: crowding --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hub", "repeats"])
def test_crowded_graphs_keep_step_records(name):
    g = hub_graph() if name == "hub" else G.synth_repeats(3000, 6, 5, 200, 150, 16)
    _, _, a, b = np_crowding(g)
    assert b.max() >= 1
    ctx = hip.Context(g)
    ctx.setup_1d(_ygs(g, 2, 10_000), hip.make_config(n_streams=64, flags=B64))
    assert ctx.record_bytes() == 16
    ctx.kshift(set=63)                                         # no a counts any more; b still does
    assert ctx.record_bytes() == 16
    ctx.close()


def test_record_width_follows_the_crowding_onset():
    g, p, _ = _t1()
    ctx = hip.Context(g)
    assert ctx.record_bytes() == 0                             # not set up
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64))
    assert ctx.kshift() == 7 and ctx.record_bytes() == 8
    assert ctx.kshift(set=2) == 2 and ctx.record_bytes() == 8  # a.max() = 2: still nothing crowded
    assert ctx.kshift(set=1) == 1 and ctx.record_bytes() == 16
    assert ctx.kshift(set=-1) == 7 and ctx.record_bytes() == 8
    for flags in (hip.F_BUNDLE(32), hip.F_BUNDLE(1), B64 | hip.F_FULL_RECORDS):
        ctx.setup_1d(p, hip.make_config(n_streams=64, flags=flags))
        assert ctx.record_bytes() == 16
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64))   # the array outlives the setups that do not use it
    assert ctx.record_bytes() == 8
    ctx.close()


# ---- T4: many waves ------------------------------------------------------------------------------------------------------
def test_full_width_window_graph_keeps_its_chain_order():
    g = G.synth_windows(20_000, 8, 12_500, 1)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    orders = {}
    for flags in (0, hip.F_FULL_RECORDS):
        ctx = hip.Context(g)
        ctx.setup_1d(p, hip.make_config(flags=flags))
        width = ctx.record_bytes()
        ctx.init_positions()
        ctx.run()
        st = ctx.stats()
        x = ctx.download()
        ctx.close()
        assert width == (16 if flags else 8) and st.bundle == 64 and st.n_streams > 64 and st.launches == 1
        assert st.term_updates == (p.iter_max + 1) * p.min_term_updates
        ids = g.node_ids[hip.sort_order(x).astype(np.int64)].astype(np.int64)
        orders[flags] = ids
        assert np.array_equal(ids, np.arange(1, g.n_nodes + 1)) or np.array_equal(ids, np.arange(g.n_nodes, 0, -1))


def test_a_layout_setup_gives_the_trip_records_back():
    """No layout kernel reads trip records: gfs_ctx_setup_nd frees them, and a later 1D setup of that context runs on step records."""
    g, p, _ = _t1()
    lp = P.LayoutSGDParams.from_graph(g, 2, 1)
    lp.iter_max, lp.min_term_updates = 1, 5_000
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64))
    assert ctx.record_bytes() == 8
    ctx.setup_nd(lp, hip.make_config(n_streams=64))
    assert ctx.record_bytes() == 16
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=B64))
    assert ctx.record_bytes() == 16
    ctx.close()
