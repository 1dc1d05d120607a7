"""The batched quality read-out (K7g, batch_quality_kernels.hip): gfs_batch_pair_errors gives, for every item of a batch of sorts
or of layouts in one step launch and one reduce launch, what gfs_ctx_pair_errors gives one item at a time — field for field,
the doubles as bits — and touches nothing.  The batch mixes items of one and of two workgroups per step distance (chains of 2048
and 2049 steps: Q_BLOCK * Q_PAIRS_PER_THREAD = 2048) with DRB1's 18; the figures are also held to the plain restatement of
tests/quality_restatement.py, within the tolerance test_gpu_quality_readout.py uses for that comparison."""
import numpy as np
import pytest

from util import G, P, load
from gfasort_amd import hip
from quality_restatement import np_pair_errors, noisy_start

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")
# 1; a mid value; n_steps - 1 of the 2048-step chain; n_steps of it (no pair there, one in the 2049-step chain); beyond lil's steps
ZS = (1, 37, 2047, 2048, 300)


def _chain(n, seed):
    """One path over n nodes of lengths 1..16, whose S lines come in another order than the path visits them."""
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


def _graphs():
    return [_chain(2048, 1), load("DRB1-3123.gfa"), _chain(2049, 2), load("lil.gfa")]


def _batch(dims, graphs, n_streams=0):
    """Set-up contexts with noisy start positions and their batch, after one run of the batch (n_streams = 0: the policy's width)."""
    ctxs = []
    for i, g in enumerate(graphs):
        ctx = hip.Context(g)
        if dims:
            p = P.LayoutSGDParams.from_graph(g, dims, 1)
        else:
            p = P.YgsParams.from_graph(g, 0, 1).path_sgd
        p.iter_max = 2
        p.seed = 9399220 + i
        assert (ctx.setup_nd if dims else ctx.setup_1d)(p, hip.make_config(n_streams=n_streams)) == hip.OK
        ctx.upload(noisy_start(g, dims, 31 + i))
        ctxs.append(ctx)
    b = hip.Batch(ctxs)
    b.run()
    return ctxs, b


@pytest.fixture(scope="module", params=[0, 2])
def resident(request):
    """(dims, graphs, contexts, batch) after a run, built once per kind and only read."""
    graphs = _graphs()
    assert [g.n_steps for g in graphs[::2]] == [2048, 2049] and graphs[3].n_steps <= 300 < graphs[1].n_steps
    ctxs, b = _batch(request.param, graphs)
    yield request.param, graphs, ctxs, b
    b.close()
    for c in ctxs:
        c.close()


def test_rows_are_the_items_own_bit_for_bit(resident):
    dims, graphs, ctxs, b = resident
    rows, ms = b.pair_errors(ZS, return_ms=True)
    print("dims", dims, "pair errors of", len(ctxs), "items at", len(ZS), "step distances: kernel_ms", ms)
    assert rows.shape == (len(ctxs), len(ZS)) and rows.dtype == hip.PAIR_ERROR_DTYPE and ms > 0.0
    for i, c in enumerate(ctxs):
        own = c.pair_errors(ZS)
        for name in hip.PAIR_ERROR_DTYPE.names:                        # field for field; the doubles as bits
            assert np.array_equal(rows[i][name].view(np.uint64), own[name].view(np.uint64)), (dims, i, name)
    # zero pairs where an item is too short, ordinary figures beside it
    assert rows[0][3]["pairs"] == 0 and rows[0][3]["sum_sq"] == 0.0 and rows[2][3]["pairs"] == 1 and rows[1][3]["pairs"] > 1000
    assert rows[3][4]["pairs"] == 0 and rows[0][2]["pairs"] == 1 and all(rows[i][0]["pairs"] > 0 for i in range(4))
    again = b.pair_errors(ZS)
    assert again.tobytes() == rows.tobytes()                           # the same call, the same bits
    one = b.pair_errors(ZS[1:2])                                       # another list: another grid, the same figures
    assert all(one[i][0].tobytes() == rows[i][1].tobytes() for i in range(4))


def test_rows_match_the_restatement(resident):
    dims, graphs, ctxs, b = resident
    rows = b.pair_errors(ZS)
    for i, (g, c) in enumerate(zip(graphs, ctxs)):
        coords = c.download()
        for r in rows[i]:
            want = np_pair_errors(g, coords, dims, int(r["step_distance"]))
            n = want["pairs"]
            print(f"dims={dims} item={i} z={int(r['step_distance'])} pairs={int(r['pairs'])}/{n}",
                  *(f"{k}: {float(r[k])!r} vs {want[k]!r}" for k in SUMS + ("max_rel_sq",)))
            assert int(r["pairs"]) == n
            assert float(r["max_rel_sq"]) == want["max_rel_sq"]
            for k in SUMS:
                assert abs(float(r[k]) - want[k]) <= n * U * abs(want[k]), (dims, i, k, int(r["step_distance"]))


@pytest.mark.parametrize("dims", [0, 2])
def test_read_outs_leave_the_state_alone(dims):
    """Positions, counters and a following run() with the read-outs in between are those without them."""
    graphs = [_chain(2049, 2), load("lil.gfa"), load("simple.gfa")]
    ctxs, b = _batch(dims, graphs, n_streams=1)                        # one stream: a run is a function of its start
    plain, pb = _batch(dims, graphs, n_streams=1)
    counters = lambda c: (c.stats().term_updates, c.stats().attempts, c.stats().iterations, c.stats().launches)
    before = [(c.download(), counters(c)) for c in ctxs]
    b.pair_errors(ZS)
    if dims:
        b.coords()
    b.pair_errors((1, 2, 3))
    for c, (x, st) in zip(ctxs, before):
        assert np.array_equal(c.download().view(np.uint64), x.view(np.uint64)) and counters(c) == st
    b.run()
    pb.run()
    for c, q in zip(ctxs, plain):
        assert np.array_equal(c.download().view(np.uint64), q.download().view(np.uint64)) and counters(c) == counters(q)
        assert counters(c)[2:] == (6, 2)
    b.close()
    pb.close()


def test_argument_rules_are_the_contexts(resident):
    dims, graphs, ctxs, b = resident
    L = hip.lib()
    n = len(ctxs)
    out = np.zeros((n, 2), dtype=hip.PAIR_ERROR_DTYPE)
    zs = np.array([1, 2], dtype=np.uint64)
    assert L.gfs_batch_pair_errors(b._h, None, 2, out.ctypes.data, None, None) == E_ARG
    assert L.gfs_batch_pair_errors(b._h, zs.ctypes.data, 2, None, None, None) == E_ARG
    zero = np.array([1, 0], dtype=np.uint64)
    assert L.gfs_batch_pair_errors(b._h, zero.ctypes.data, 2, out.ctypes.data, None, None) == E_ARG
    assert b"step distance of 0" in L.gfs_last_error()
    assert L.gfs_batch_pair_errors(b._h, zs.ctypes.data, 65536, out.ctypes.data, None, None) == E_ARG
    assert L.gfs_batch_pair_errors(b._h, None, 0, None, None, None) == 0            # nothing asked, nothing done
    assert not out.view(np.uint8).any()                                             # (no refused call wrote anything)
    assert b.pair_errors(np.zeros(0, dtype=np.uint64)).shape == (n, 0)
