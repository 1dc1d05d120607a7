"""The oracle's mirror of the product's crowding rule (sgd_device.h crowd_shift) — CPU only.

The reference has no crowding; the product scales a term's mu by 2^-k where nodes are crowded.  The oracle computes the
per-node exponents itself (a sliding window per path, not the kernel's look-back) and applies the scale in its state API
when asked (O.State(..., crowd_kshift=k)); the one-shot and threaded modes, which restate the reference, never do.
Here: the exponents against a numpy restatement on adversarial graphs, and the mirror's switch — off is the old oracle bit
for bit, an onset above every exponent is off, kshift = 0 changes the result."""
import hashlib

import numpy as np
import pytest

from util import O, G, P, load, oracle_graph, oracle_params, gaussian_init, crowding_edge_graph, hub_graph, np_crowding


def _graphs():
    return {
        "edge": crowding_edge_graph()[0],
        "repeats_p1": G.synth_repeats(3000, 6, 1, 200, 150, 11),
        "repeats_p5": G.synth_repeats(3000, 6, 5, 200, 150, 12),
        "hub": hub_graph(),
        "DRB1": load("DRB1-3123.gfa"),
        "windows": G.synth_windows(5000, 8, 2500, 4),
    }


@pytest.mark.parametrize("name", ["edge", "repeats_p1", "repeats_p5", "hub", "DRB1", "windows"])
def test_node_crowding_equals_numpy_restatement(name):
    g = _graphs()[name]
    cnt, rep, a, b = np_crowding(g)
    oa, ob = O.node_crowding(oracle_graph(g))
    assert np.array_equal(oa.astype(np.int64), a) and np.array_equal(ob.astype(np.int64), b)
    if name == "edge":
        _, expect = crowding_edge_graph()
        for what, (n, c, r) in expect.items():
            assert (cnt[n], rep[n]) == (c, r), what
        assert a.max() == 17 and b.max() == 6                       # the hub, the 64-fold repeat
    if name.startswith("repeats"):                                 # copies up to 200: some window holds 64 / period visits
        assert b.max() == (6 if name == "repeats_p1" else 4)


def test_node_crowding_premises_of_the_edge_graph():
    """What each edge case is there for, in exponents: distance 63 counts and 64 does not, a path boundary does not, 2^k
    and 2^k + 1 round up, absent steps have none."""
    g, expect = crowding_edge_graph()
    oa, ob = O.node_crowding(oracle_graph(g))
    want = {"dist63": (1, 1), "dist64": (1, 0), "path_edge": (1, 0), "no_node_window": (2, 2), "cnt16": (4, 0),
            "cnt17": (5, 0), "cnt32": (5, 0), "cnt33": (6, 0), "rep2": (1, 1), "rep4": (2, 2), "rep5": (3, 3),
            "rep8": (3, 3), "rep9": (4, 4), "rep64": (6, 6), "hub": (17, 4)}
    for what, (n, _, _) in expect.items():
        assert (int(oa[n]), int(ob[n])) == want[what], what


def _ygs(g, iter_max, mtu=None):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    if mtu:
        p.min_term_updates = mtu
    return p


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8)).hexdigest()[:16]


def _state_runs(crowd):
    """Four state-API runs (reference streams 1D and 2D, the team mirror 1D and 3D) with crowding `crowd`; digests."""
    out = {}
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    p = _ygs(g, 3)
    x = O.init_positions(og)
    O.State(og, oracle_params(p), n_streams=4, crowd_kshift=crowd).run(x)
    out["ref_1d"] = _digest(x)
    pl = P.LayoutSGDParams.from_graph(g, 2, 1)
    pl.iter_max, pl.min_term_updates = 2, 8000
    c = gaussian_init(g, 2, 7)
    O.State(og, oracle_params(pl), dims=2, n_streams=1, crowd_kshift=crowd).run(c)
    out["ref_2d"] = _digest(c)
    from gfasort_amd.distributed import path_order_layout
    gr = G.synth_repeats(6000, 8, 1, 40, 200, 3)
    ogr = oracle_graph(gr)
    p = _ygs(gr, 3, 60_000)
    x = O.init_positions(ogr)
    O.State(ogr, oracle_params(p), n_streams=64, bundle=64, node_slots=path_order_layout(gr), chain=64, partners=2,
            crowd_kshift=crowd).run(x)
    out["team_1d"] = _digest(x)
    pl = P.LayoutSGDParams.from_graph(gr, 3, 1)
    pl.iter_max, pl.min_term_updates = 2, 40_000
    c = gaussian_init(gr, 3, 5)
    O.State(ogr, oracle_params(pl), dims=3, n_streams=64, bundle=64, node_slots=path_order_layout(gr), chain=16,
            partners=2, crowd_kshift=crowd).run(c)
    out["team_3d"] = _digest(c)
    return out


# the oracle before it had a crowding mirror, on the runs of _state_runs (recorded once; a change of the state API's default
# behaviour changes them)
_BEFORE = {"ref_1d": "00b76280ec6f2418", "ref_2d": "1b6e650c91788726", "team_1d": "1364f3555904143f", "team_3d": "91777827371664d5"}


def test_crowding_off_is_the_state_api_of_before():
    assert _state_runs(None) == _BEFORE


def test_an_onset_above_every_exponent_is_off_on_graphs_without_repeats():
    """kshift > max a and b = 0 everywhere: k = 0 for every term, in both rules, and nothing may round differently."""
    for g in (load("DRB1-3123.gfa"), G.synth_windows(5000, 8, 2500, 4)):
        og = oracle_graph(g)
        a, b = O.node_crowding(og)
        assert b.max() == 0 and a.max() >= 1
        from gfasort_amd.distributed import path_order_layout
        for kw in (dict(n_streams=3), dict(n_streams=64, bundle=64, node_slots=path_order_layout(g), chain=64, partners=2)):
            p = _ygs(g, 2, 20_000)
            xs = []
            for crowd in (None, int(a.max()), 40):
                x = O.init_positions(og)
                O.State(og, oracle_params(p), crowd_kshift=crowd, **kw).run(x)
                xs.append(x.view(np.uint64))
            assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[0], xs[2])
            pl = P.LayoutSGDParams.from_graph(g, 2, 1)
            pl.iter_max, pl.min_term_updates = 2, 20_000
            cs = []
            for crowd in (None, int(a.max())):
                c = gaussian_init(g, 2, 3)
                O.State(og, oracle_params(pl), dims=2, crowd_kshift=crowd,
                        **{**kw, "chain": 16 if "bundle" in kw else 1}).run(c)
                cs.append(c.view(np.uint64))
            assert np.array_equal(cs[0], cs[1])


@pytest.mark.parametrize("dims", [0, 2])
def test_kshift_zero_changes_a_single_stream(dims):
    """The mirror is not a no-op: at kshift = 0 every term between visited nodes of a > 0 is scaled."""
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    assert O.node_crowding(og)[0].max() >= 3
    runs = []
    for crowd in (None, 0):
        if dims:
            pl = P.LayoutSGDParams.from_graph(g, dims, 1)
            pl.iter_max, pl.min_term_updates = 2, 8000
            x = gaussian_init(g, dims, 7)
            O.State(og, oracle_params(pl), dims=dims, n_streams=1, crowd_kshift=crowd).run(x)
        else:
            x = O.init_positions(og)
            O.State(og, oracle_params(_ygs(g, 2, 8000)), n_streams=1, crowd_kshift=crowd).run(x)
        runs.append(x)
    assert np.isfinite(runs[1]).all()
    assert (runs[0].view(np.uint64) != runs[1].view(np.uint64)).mean() > 0.5
