"""The 16-byte step records (index_set_kernels.hip K3, format sgd_device.h) and the crowding rule that reads them, exactly.

G1  every record field by field against a numpy restatement of K3 (index_ref.py): node slot, path id and reverse bit, the 55-bit
    position, the crowding exponents a (steps on the node) and b (visits within 64 consecutive steps of a path), the zeroed padding
    record; and the shapes at which a single context, built as a union of one item, can still go wrong.
G2  the crowding onset kshift the kernels are handed, and its per-context override.
G3  reference streams with kshift = 0 (the `a` rule) on one stream, 1D and nD, fused and per-iteration, == the oracle bit for bit.
G4  one team wave with kshift = 0 and 1 (the `a` rule in every trip form) == the oracle's mirror bit for bit.
G5  one team wave at the natural kshift on a graph with tandem repeats in short paths (the `b` rule) == the mirror.
G6  positions past 2^32 and 2^53 bp: records, K4, replays, the sampler, a team wave; the 2^55 bp refusal boundary.
Each test checks from the readback that what it exercises is there (some k > 0, some position >= 2^32, ...)."""
import numpy as np
import pytest

from util import (O, G, P, load, oracle_graph, oracle_params, gaussian_init, crowding_edge_graph, hub_graph, np_crowding,
                  graph_from_paths, NO_NODE)
from index_ref import POS_HI, HostIndex, np_records, same_records, free_device_bytes
from gfasort_amd import hip

pytestmark = pytest.mark.gpu


def _ygs(g, iter_max, mtu=None):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    if mtu:
        p.min_term_updates = mtu
    return _sane_space(p)


def _sane_space(p):
    """The derived space is the longest path in bp (ygs.rs): the zeta table has that many entries, which a graph of 2^53 bp
    cannot hold.  Cap it; the sampler clamps jumps to it either way."""
    p.space = min(p.space, 20_000)
    return p


def _node_slots(g):
    from gfasort_amd.distributed import path_order_layout
    return path_order_layout(g)


def _check_records(g, node_perm=None):
    crowd = np_crowding(g)
    ctx = hip.Context(g, node_perm=node_perm)
    rec = ctx.step_records()
    perm = ctx.node_layout()
    ctx.close()
    if node_perm is not None:
        assert np.array_equal(perm, node_perm)
    want = np_records(g, perm, crowd)
    assert rec.shape == (g.n_steps + 1, 4)
    same_records(rec, want)
    return rec, crowd


# ---- graphs --------------------------------------------------------------------------------------------------------
def _repeats(period):
    return G.synth_repeats(3000, 6, period, 200, 150, 11 + period)


def big_graph(n=(1 << 21) + (1 << 16), seed=9):
    """Node lengths near 2^32 - 1: path 0 walks every node (its total crosses 2^53 bp), path 1 every node but each 7th,
    reverse steps at random, path 2 a short one with an absent node.  No path visits a node twice."""
    rng = np.random.default_rng(seed)
    node_len = rng.integers((1 << 32) - (1 << 24), 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    node_len[rng.integers(0, n, 64)] = 0xFFFFFFFF
    node_len[:8] = [1, 2, 3, 0xFFFFFFFF, 5, 6, 7, 8]
    p0 = np.arange(n, dtype=np.int64)
    p1 = p0[p0 % 7 != 3]
    p2 = np.array([5, 9, NO_NODE, 11, 17, 4], dtype=np.int64)
    steps = np.concatenate([p0, p1, p2])
    first = np.array([0, p0.size, p0.size + p1.size, steps.size], dtype=np.uint64)
    return G.FlatGraph(node_len=node_len, step_node=steps.astype(np.uint32),
                       step_is_rev=(rng.random(steps.size) < 0.25).astype(np.uint8), path_first_step=first,
                       node_ids=np.arange(1, n + 1, dtype=np.uint64), path_names=["p0", "p1", "p2"])


_BIG = {}


def _big():
    if "g" not in _BIG:
        _BIG["g"] = big_graph()
    return _BIG["g"]


def boundary_graph(extra):
    """One path of 2^23 steps over 1024 nodes of 2^32 - 1 bp, then one node of 2^23 - 1 + extra bp: a total of 2^55 - 1 + extra."""
    n = 1024
    node_len = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
    node_len[n] = (1 << 23) - 1 + extra
    steps = np.concatenate([np.tile(np.arange(n, dtype=np.uint32), (1 << 23) // n), [n]]).astype(np.uint32)
    return G.FlatGraph(node_len=node_len, step_node=steps, step_is_rev=np.zeros(steps.size, dtype=np.uint8),
                       path_first_step=np.array([0, steps.size], dtype=np.uint64),
                       node_ids=np.arange(1, n + 2, dtype=np.uint64), path_names=["p0"])


# ---- G1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple.gfa", "lil.gfa", "DRB1-3123.gfa", "repeats_p1", "repeats_p5", "perm", "edge"])
def test_step_records_field_by_field(name):
    node_perm = None
    if name.endswith(".gfa"):
        g = load(name)
    elif name.startswith("repeats"):
        g = _repeats(int(name[-1]))
    elif name == "perm":
        g = load("DRB1-3123.gfa")
        node_perm = np.random.default_rng(4).permutation(g.n_nodes).astype(np.uint32)
    else:
        g, _ = crowding_edge_graph()
    rec, (cnt, rep, a, b) = _check_records(g, node_perm)
    if name.startswith("repeats"):
        assert b.max() == (6 if name == "repeats_p1" else 4)          # rep 64 (period 1) / 13 (period 5)
    if name == "edge":
        assert a.max() == 17 and b.max() == 6 and (g.step_node == NO_NODE).any()
        assert ((rec[:-1, 0] == NO_NODE) == (g.step_node == NO_NODE)).all()
    if name == "DRB1-3123.gfa":
        assert a.max() >= 3 and g.step_is_rev.any()


def test_step_records_past_2_to_the_53():
    g = _big()
    rec, _ = _check_records(g)
    pos, plen = g.step_positions()
    assert int(pos.max()) >= 1 << 53 and int(plen.max()) > 1 << 53
    assert ((rec[:-1, 3] & POS_HI) > 0).mean() > 0.9                   # the high word is in use nearly everywhere


# ---- G1b: a single context is a union of one item ---------------------------------------------------------------------
E_ARG = -1
_LONG_RUN = 40                                                         # nodes of one run of first visits


def _edge_case(name):
    """(graph, node_perm or None, refused).  Small graphs at the seams of the one-item union."""
    perm = None
    if name == "no_steps":
        g = graph_from_paths([[], []], [3, 1, 4])
    elif name == "no_paths":
        g = graph_from_paths([], [2, 3, 5])
        assert g.path_first_step.tolist() == [0]
    elif name == "empty_first_and_last_path":                           # the item's first step must still start a path
        g = graph_from_paths([[], [2, 0, 1, 0, 3], []], [3, 1, 4, 1])
    elif name == "absent_first_step":                                   # the anchor look-up at p == NO_NODE
        g = graph_from_paths([[NO_NODE, 1, 2, 0], [2, 3, 4, 0]], [3, 1, 4, 1, 5], rev=[0, 1, 0, 0, 1, 0, 0, 1])
    elif name == "branch_off_a_long_run":                               # head of the run: log2(40) > 4 rounds, a second chunk
        g = graph_from_paths([list(range(_LONG_RUN)), [_LONG_RUN // 2, _LONG_RUN, _LONG_RUN + 1, _LONG_RUN // 2 + 1]],
                             np.arange(1, _LONG_RUN + 3))
    elif name == "odd_nodes_unvisited":                                 # they go last, in index order
        g = graph_from_paths([[0, 2, 4, 6, 8], [8, 4, 10, 0]], np.arange(1, 13))
    elif name in ("given_layout", "given_layout_bad_step"):
        g = graph_from_paths([[NO_NODE, 1, 2, 0], [2, 3, 4, 0], [5, 5]], [3, 1, 4, 1, 5, 9, 2])
        perm = np.array([4, 0, 6, 2, 5, 1, 3], dtype=np.uint32)
        if name == "given_layout_bad_step":
            bad = g.step_node.copy()
            bad[5] = g.n_nodes
            g = G.FlatGraph(node_len=g.node_len, step_node=bad, step_is_rev=g.step_is_rev, path_first_step=g.path_first_step,
                            node_ids=g.node_ids, path_names=g.path_names)
    elif name == "no_nodes_no_steps":
        g = graph_from_paths([[]], [])
    elif name == "no_nodes_absent_steps":
        g = graph_from_paths([[NO_NODE, NO_NODE, NO_NODE]], [])
    elif name == "no_nodes_one_real_step":                              # refused before anything is indexed by the step's node
        g = graph_from_paths([[NO_NODE, 0]], [])
    return g, perm, name in ("given_layout_bad_step", "no_nodes_one_real_step")


EDGE_CASES = ["no_steps", "no_paths", "empty_first_and_last_path", "absent_first_step", "branch_off_a_long_run", "odd_nodes_unvisited",
              "given_layout", "given_layout_bad_step", "no_nodes_no_steps", "no_nodes_absent_steps", "no_nodes_one_real_step"]


@pytest.mark.parametrize("name", EDGE_CASES)
def test_single_context_edge_cases(name):
    """gfs_ctx_create builds its context as a union of ONE item through the set's kernels.  For each graph that builds: the layout
    is the host's (gfs_shared_node_layout) or the given one, the records are the numpy restatement's field by field, and — where a
    path has two steps or more — one reference stream, which finds its steps through the path records the DEVICE now writes,
    ends where the oracle's ends, bit for bit.  A refused graph is refused with "step_node out of range" and leaves no device
    memory behind."""
    g, node_perm, refused = _edge_case(name)
    if refused:
        hip.Context(graph_from_paths([[0, 1]], [1, 1])).close()         # (modules loaded, the runtime's pools warm)
        free = [free_device_bytes()]
        for _ in range(2):
            with pytest.raises(hip.GfsError) as ei:
                hip.Context(g, node_perm=node_perm)
            assert ei.value.code == E_ARG and "step_node out of range" in str(ei.value) and "set item" not in str(ei.value)
            del ei                                                      # (the traceback holds the frame of the failed create)
            free.append(free_device_bytes())
        print("free device memory before, after one and after two refused creates:", free)
        assert free[1] == free[0] and free[2] == free[0]
        return
    host = HostIndex(g)
    ctx = hip.Context(g, node_perm=node_perm)
    try:
        if node_perm is None:
            host.check(ctx, name)
        else:
            assert np.array_equal(ctx.node_layout(), node_perm)
            assert not np.array_equal(node_perm, host.layout)           # (the given layout is not the one the device would derive)
            same_records(ctx.step_records(), np_records(g, node_perm, host.crowd), name)
        if name == "odd_nodes_unvisited":
            odd = np.arange(1, g.n_nodes, 2)
            assert ctx.node_layout()[odd].tolist() == list(range(g.n_nodes - odd.size, g.n_nodes))
        if name == "branch_off_a_long_run":                             # the branch sits right after the node it branches off
            lay = ctx.node_layout()
            assert lay[_LONG_RUN] == lay[_LONG_RUN // 2] + 1 and lay[_LONG_RUN + 1] == lay[_LONG_RUN // 2] + 2
        if g.n_nodes == 0 or np.diff(g.path_first_step.astype(np.int64)).max(initial=0) < 2:
            return
        p = _ygs(g, 1, 300)
        og = oracle_graph(g)
        x_ref = O.init_positions(og)
        rc, st, _ = O.sgd_1d(og, oracle_params(p), x_ref, n_streams=1)
        ctx.setup_1d(p, hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1)))
        ctx.init_positions()
        ctx.run()
        hst = ctx.stats()
        x = ctx.download()
        assert rc == 0 and hst.term_updates == st.term_updates == 2 * 300 and hst.attempts == st.attempts
        assert np.array_equal(x.view(np.uint64), x_ref.view(np.uint64))
        assert not np.array_equal(x, hip.init_positions(g))             # (the stream moved something)
    finally:
        ctx.close()


# ---- G2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [0, 1, 2, 3, 31, 32])
def test_kshift_policy_and_override(per):
    T = 64
    S = max(per * 2 * T + (17 if per else 100), 2)
    g = graph_from_paths([list(range(S))], np.full(S, 3))
    assert S // (2 * T) == per
    ctx = hip.Context(g)
    ctx.setup_1d(_ygs(g, 1, 1000), hip.make_config(n_streams=T, flags=hip.F_BUNDLE(1)))
    want = int(np.floor(np.log2(max(per, 1)))) + 2
    assert ctx.kshift() == want
    assert ctx.kshift(set=0) == 0 and ctx.kshift() == 0
    assert ctx.kshift(set=want + 3) == want + 3
    assert ctx.kshift(set=-1) == want
    ctx.close()


# ---- G3 ----------------------------------------------------------------------------------------------------------
def _g3_graph(name):
    return {"DRB1": lambda: load("DRB1-3123.gfa"), "repeats": lambda: _repeats(1), "hub": lambda: hub_graph()}[name]()


@pytest.mark.parametrize("name", ["DRB1", "repeats", "hub"])
@pytest.mark.parametrize("dims", [0, 2, 3, 8])
def test_reference_streams_a_rule_on_one_stream_equal_the_oracle(name, dims):
    """One stream has no concurrency: with kshift = 0 every term is scaled by 2^-max(a_i, a_j), b is ignored (b > 0 on the
    repeat graph), and K1 / K1d (1D) and K2 / K2d (nD) must equal the oracle's state with crowd_kshift = 0 bit for bit."""
    g = _g3_graph(name)
    og = oracle_graph(g)
    _, _, a, b = np_crowding(g)
    assert a.max() >= 3
    if name == "repeats":
        assert b.max() >= 1
    if dims:
        p = P.LayoutSGDParams.from_graph(g, dims, 1)
        p.iter_max, p.min_term_updates = 3, 12_000
        x0 = gaussian_init(g, dims, 7)
    else:
        p = _ygs(g, 3, 12_000)
        x0 = hip.init_positions(g)
    op = oracle_params(p)
    x_ref = x0.copy()
    O.State(og, op, dims=dims, n_streams=1, crowd_kshift=0).run(x_ref)
    x_off = x0.copy()
    O.State(og, op, dims=dims, n_streams=1).run(x_off)
    assert not np.array_equal(x_ref.view(np.uint64), x_off.view(np.uint64))     # the scale is reached
    for extra, launches in ((0, 1), (hip.F_NO_FUSE, 4)):
        ctx = hip.Context(g)
        cfg = hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1) | extra)
        (ctx.setup_nd if dims else ctx.setup_1d)(p, cfg)
        assert ctx.kshift(set=0) == 0
        ctx.upload(x0)
        ctx.run()
        st = ctx.stats()
        x = ctx.download()
        ctx.close()
        assert st.bundle == 1 and st.launches == launches and st.term_updates == 4 * 12_000
        assert np.array_equal(x.view(np.uint64), x_ref.view(np.uint64)), f"flags {extra:#x}"


# ---- G4 / G5: one team wave against the mirror ------------------------------------------------------------------------
VARIANTS_1D = [(False, True, 2, True), (True, True, 2, True), (True, False, 2, True), (True, True, 2, False),
               (True, True, 1, True), (False, True, 1, True)]
VARIANTS_ND = [(2, True), (2, False), (1, True)]


def _team_1d(g, kshift, fused, fused_trip, partners, twin, iter_max=4, mtu=100_000, natural=False):
    p = _ygs(g, iter_max, mtu)
    flags = (hip.F_BUNDLE(64) | (0 if fused else hip.F_NO_FUSE) | (0 if fused_trip else hip.F_DBG_NO_FUSED_TRIP) |
             (0 if partners == 2 else hip.F_ONE_PARTNER) | (0 if twin else hip.F_DBG_NO_TWIN_TRIP))
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=64, flags=flags))
    ks = ctx.kshift() if natural else ctx.kshift(set=kshift)
    ctx.upload(hip.init_positions(g))
    ctx.run()
    hst = ctx.stats()
    x = ctx.download()
    ctx.close()
    og = oracle_graph(g)
    st_o = O.State(og, oracle_params(p), n_streams=64, bundle=64, node_slots=_node_slots(g), chain=64, fused_trip=fused_trip,
                   partners=partners, twin_trip=twin, crowd_kshift=ks)
    x_ref = O.init_positions(og)
    st_o.run(x_ref)
    so = st_o.stats()
    assert hst.launches == (1 if fused else iter_max + 1)
    assert (hst.term_updates, hst.attempts) == (so.term_updates, so.attempts) and hst.term_updates == (iter_max + 1) * mtu
    assert np.array_equal(x.view(np.uint64), x_ref.view(np.uint64))
    return ks


def _team_nd(g, dims, kshift, partners, twin, iter_max=3, mtu=80_000, natural=False):
    p = _sane_space(P.LayoutSGDParams.from_graph(g, dims, 1))
    p.iter_max, p.min_term_updates = iter_max, mtu
    c0 = gaussian_init(g, dims, 5)
    ctx = hip.Context(g)
    ctx.setup_nd(p, hip.make_config(n_streams=64, flags=hip.F_BUNDLE(64) | (0 if partners == 2 else hip.F_ONE_PARTNER) |
                                    (0 if twin else hip.F_DBG_NO_TWIN_TRIP)))
    ks = ctx.kshift() if natural else ctx.kshift(set=kshift)
    ctx.upload(c0)
    ctx.run()
    hst = ctx.stats()
    c = ctx.download()
    ctx.close()
    og = oracle_graph(g)
    c_ref = c0.copy()
    st_o = O.State(og, oracle_params(p), dims=dims, n_streams=64, bundle=64, node_slots=_node_slots(g), chain=16,
                   partners=partners, twin_trip=twin, crowd_kshift=ks)
    st_o.run(c_ref)
    so = st_o.stats()
    assert (hst.term_updates, hst.attempts) == (so.term_updates, so.attempts) and hst.term_updates == (iter_max + 1) * mtu
    assert np.array_equal(c.view(np.uint64), np.ascontiguousarray(c_ref).ravel().view(np.uint64))
    return ks


_G4 = {}


def _g4_graph(name):
    if name not in _G4:
        _G4[name] = G.synth_windows(40_000, 8, 20_000, 12) if name == "windows" else G.synth_bubbles(30_000, 8, 3)
    return _G4[name]


@pytest.mark.parametrize("kshift", [0, 1])
@pytest.mark.parametrize("graph", ["windows", "bubbles"])
@pytest.mark.parametrize("fused,fused_trip,partners,twin", VARIANTS_1D)
def test_team_kernel_a_rule_equals_the_mirror(graph, fused, fused_trip, partners, twin, kshift):
    """No node repeats within a path (b = 0): trips are node-disjoint and a (0..3) alone decides k."""
    g = _g4_graph(graph)
    _, _, a, b = np_crowding(g)
    assert b.max() == 0 and a.max() - kshift >= 2
    _team_1d(g, kshift, fused, fused_trip, partners, twin)


@pytest.mark.parametrize("kshift", [0, 1])
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("partners,twin", VARIANTS_ND)
def test_layout_team_kernel_a_rule_equals_the_mirror(dims, partners, twin, kshift):
    g = _g4_graph("windows")
    _, _, a, b = np_crowding(g)
    assert b.max() == 0 and a.max() - kshift >= 2
    _team_nd(g, dims, kshift, partners, twin)


def repeats_in_short_paths(seed=12):
    """The windows graph plus short paths (< 2B = 128 steps, so lane 0 alone takes their terms) that step repeatedly on
    nodes of the long paths: visits 2, 3, 4, 5 and 9 within 64 steps (b = 1, 2, 2, 3, 4), a pair at distance 63 (b = 1) and
    one at distance 64 (b = 0).  Returns (graph, {node: expected b})."""
    g = G.synth_windows(40_000, 8, 20_000, 12)
    rng = np.random.default_rng(seed)
    long_nodes = rng.permutation(np.unique(g.step_node))
    it = iter(long_nodes.tolist())
    paths, want = [], {}
    for r, bb in ((2, 1), (3, 2), (4, 2), (5, 3), (9, 4)):
        x = next(it)
        pth = [next(it) for _ in range(3)]
        for _ in range(r):
            pth += [x] + [next(it) for _ in range(4)]
        paths.append(pth)
        want[x] = bb
    for dist, bb in ((63, 1), (64, 0)):
        x = next(it)
        paths.append([next(it)] + [x] + [next(it) for _ in range(dist - 1)] + [x] + [next(it)])
        want[x] = bb
    assert all(len(pth) < 128 for pth in paths)
    extra = np.concatenate([np.asarray(pth, dtype=np.uint32) for pth in paths])
    first = np.concatenate([g.path_first_step, g.path_first_step[-1] + np.cumsum([len(pth) for pth in paths]).astype(np.uint64)])
    g2 = G.FlatGraph(node_len=g.node_len, step_node=np.concatenate([g.step_node, extra]),
                     step_is_rev=np.zeros(g.n_steps + extra.size, dtype=np.uint8), path_first_step=first.astype(np.uint64),
                     node_ids=g.node_ids, path_names=g.path_names + [f"r{i}" for i in range(len(paths))])
    return g2, want


@pytest.mark.parametrize("variant", range(len(VARIANTS_1D) + 2 * len(VARIANTS_ND)))
def test_team_kernel_b_rule_at_the_natural_kshift_equals_the_mirror(variant):
    """b decides k (a - kshift <= 0 everywhere at the product's own onset), in every trip form, 1D and nD; a lone lane of a
    short path may pair a node with itself (i == j)."""
    g, want = repeats_in_short_paths()
    _, _, a, b = np_crowding(g)
    for n, bb in want.items():
        assert b[n] == bb, (n, b[n], bb)
    ctx = hip.Context(g)
    rec = ctx.step_records()
    ctx.close()
    assert ((rec[:-1, 3] >> 29) & 7).max() == 4
    if variant < len(VARIANTS_1D):
        ks = _team_1d(g, None, *VARIANTS_1D[variant], natural=True)
    else:
        v = variant - len(VARIANTS_1D)
        ks = _team_nd(g, 2 + v // len(VARIANTS_ND), None, *VARIANTS_ND[v % len(VARIANTS_ND)], natural=True)
    assert a.max() - ks <= 0 and b.max() >= 1


# ---- G6: positions past 2^32 and 2^53 bp -------------------------------------------------------------------------------
def test_device_initial_positions_past_2_to_the_53():
    g = _big()
    assert int(g.node_len.astype(np.uint64).sum()) > 1 << 53
    ctx = hip.Context(g)
    ctx.setup_1d(_ygs(g, 1, 1000), hip.make_config(n_streams=64))
    ctx.init_positions()
    x = ctx.download()
    ctx.close()
    want = hip.init_positions(g)
    assert want.max() > 2.0 ** 53
    assert np.array_equal(x.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(want, np.concatenate([[0], np.cumsum(g.node_len.astype(np.uint64))[:-1]]).astype(np.float64))


@pytest.mark.parametrize("dims", [0, 2])
def test_single_stream_replay_past_2_to_the_53(dims):
    g = _big()
    og = oracle_graph(g)
    if dims:
        p = _sane_space(P.LayoutSGDParams.from_graph(g, dims, 1))
        p.iter_max, p.min_term_updates = 2, 6000
        c0 = gaussian_init(g, dims, 3)
        c_ref = c0.copy()
        rc, st, _ = O.sgd_nd(og, oracle_params(p), c_ref, n_streams=1)
        rc2, x, hst = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1)))
    else:
        p = _ygs(g, 2, 6000)
        c_ref = O.init_positions(og)
        rc, st, _ = O.sgd_1d(og, oracle_params(p), c_ref, n_streams=1)
        rc2, x, hst = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1)))
    assert rc == 0 and rc2 == 0
    assert hst.term_updates == st.term_updates == 3 * 6000 and hst.attempts == st.attempts
    assert np.abs(c_ref).max() > 2.0 ** 53
    assert np.array_equal(x.view(np.uint64), np.ascontiguousarray(c_ref).ravel().view(np.uint64))


def test_sampler_trace_full_width_past_2_to_the_53():
    g = _big()
    p = _ygs(g, 2, 4096 * 30)
    T, K = 4096, 20
    og = oracle_graph(g)
    x_ref = O.init_positions(og)
    rc, st, tr_ref = O.sgd_1d(og, oracle_params(p), x_ref, n_streams=T, trace_per_stream=K)
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=T, trace_per_stream=K, flags=hip.F_BUNDLE(1)))
    ctx.upload(hip.init_positions(g))
    ctx.run()
    tr, counts = ctx.trace()
    hst = ctx.stats()
    ctx.close()
    tr_ref = tr_ref.reshape(T, K)
    assert hst.term_updates == st.term_updates and hst.attempts == st.attempts
    assert tr_ref["d_ij"].max() > 2.0 ** 32
    assert np.array_equal(tr["i"], tr_ref["i"]) and np.array_equal(tr["j"], tr_ref["j"])
    assert np.array_equal(tr["d_ij"].view(np.uint64), tr_ref["d_ij"].view(np.uint64))


@pytest.mark.parametrize("dims", [0, 2])
def test_team_wave_past_2_to_the_53_equals_the_mirror(dims):
    g = _big()
    if dims:
        _team_nd(g, dims, None, 2, True, iter_max=2, mtu=60_000, natural=True)
    else:
        _team_1d(g, None, True, True, 2, True, iter_max=2, mtu=60_000, natural=True)


def test_the_2_to_the_55_boundary():
    """A path of 2^55 - 1 bp is accepted — its last records carry high word 0x7FFFFF — and replays like the oracle for a
    short iteration; one of 2^55 bp is refused."""
    g = boundary_graph(0)
    pos, plen = g.step_positions()
    assert int(plen[0]) == (1 << 55) - 1 and int(pos[-1]) >> 32 == POS_HI
    ctx = hip.Context(g)
    rec = ctx.step_records()
    ctx.close()
    hi = (rec[:-1, 3] & POS_HI).astype(np.int64)
    assert np.array_equal(hi, (pos >> np.uint64(32)).astype(np.int64)) and hi[-1] == POS_HI
    assert np.array_equal(rec[:-1, 2], (pos & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert ((rec[:-1, 3] >> 23) & 63)[0] == 13 and not rec[-1].any()   # 2^13 visits per node
    p = _ygs(g, 1, 3000)
    og = oracle_graph(g)
    x_ref = O.init_positions(og)
    rc, st, _ = O.sgd_1d(og, oracle_params(p), x_ref, n_streams=1)
    rc2, x, hst = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1, flags=hip.F_BUNDLE(1)))
    assert rc == rc2 == 0 and hst.term_updates == st.term_updates == 2 * 3000
    assert np.array_equal(x.view(np.uint64), x_ref.view(np.uint64))
    with pytest.raises(hip.GfsError) as e:
        hip.Context(boundary_graph(1))
    assert e.value.code == -5 and "2^55" in str(e.value)
