"""The batch read-out (K4b / K6b, batch_readout_kernels.hip): gfs_batch_init_positions and gfs_batch_results give, for every item
of a batch in one launch, what gfs_ctx_init_positions, gfs_ctx_download_positions and gfs_ctx_sort_order give one item at a time.
Every expectation is the host's std::stable_sort (hip.sort_order) on downloaded positions, or the item's own context calls (the
rocPRIM path): the kernel under test is never compared with itself."""
import functools
import time

import numpy as np
import pytest

from util import O, G, P, load, oracle_graph, oracle_params
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

FIXTURES = (("simple.gfa", 100), ("lil.gfa", 100), ("DRB1-3123.gfa", 10))
E_ARG, E_UNSUPPORTED = -1, -5
SEAM_SIZES = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4955, 8191, 8192, 8193)


def _ygs(g, iter_max, seed=None):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    if seed is not None:
        p.seed = seed
    return p


def _chain(n, seed):
    """One path over n nodes of lengths 1..16, whose S lines come in another order than the path visits them."""
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    if n > 1 and np.array_equal(s_order, np.arange(1, n + 1)):
        s_order = s_order[::-1]
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


def _crafted(n, seed):
    """Positions with what a sort can get wrong: blocks of bit-equal values, both zeros, negatives, infinities, denormals, NaNs."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1000.0, n)
    x[rng.integers(0, n, max(1, n // 3))] = 7.25                       # one value, scattered: ties fall by dense index
    if n >= 8:
        a = int(rng.integers(0, n - 4))
        x[a:a + 4] = -3.5                                              # a block of equal negatives
    picks = rng.permutation(n)
    special = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.0 ** -1060, np.nan, 0.0, -0.0, np.nan, -1.0, np.nan]
    for k, v in zip(picks, special):                                   # (as many as the graph has room for)
        x[k] = v
    return x


def _ctx(g, p, **cfg):
    ctx = hip.Context(g)
    rc = ctx.setup_1d(p, hip.make_config(**cfg))
    return ctx, rc


@pytest.fixture(scope="module")
def seams():
    """The seams batch, built once and only read: (contexts, the positions uploaded to them, batch)."""
    graphs = [_chain(n, 100 + n) for n in SEAM_SIZES[:8]]
    graphs += [load("lil.gfa"), G.parse_gfa("S\t1\tAC\nS\t2\tG\nP\ta\t1+\t*\nP\tb\t2+\t*\n"), load("simple.gfa")]   # idle in the middle
    graphs += [_chain(n, 100 + n) for n in SEAM_SIZES[8:]]
    ctxs, xs = [], []
    for i, g in enumerate(graphs):
        ctx, rc = _ctx(g, _ygs(g, 2), n_streams=1)
        idle = rc == hip.NOTHING_TO_DO
        assert idle == (i == 9)
        x = _crafted(g.n_nodes, 7000 + i)
        ctx.upload(x)
        ctxs.append(ctx)
        xs.append(x)
    assert any(not np.array_equal(c.node_layout(), np.arange(c.graph.n_nodes)) for c in ctxs)   # positions do get gathered
    b = hip.Batch(ctxs)
    yield ctxs, xs, b
    b.close()
    for c in ctxs:
        c.close()


def _check_against_contexts(ctxs, xs, positions, orders):
    for i, ctx in enumerate(ctxs):
        n = ctx.graph.n_nodes
        x = ctx.download()
        assert np.array_equal(x.view(np.uint64), xs[i].view(np.uint64)), i          # (the upload, NaN payloads included)
        want = hip.sort_order(x)
        if positions is not None:
            assert positions[i].dtype == np.float64 and np.array_equal(positions[i].view(np.uint64), x.view(np.uint64)), (i, n)
        if orders is not None:
            assert orders[i].dtype == np.uint64 and orders[i].shape == (n,)
            assert np.array_equal(orders[i], want), (i, n)
            assert np.array_equal(orders[i], ctx.sort_order()), (i, n)


def test_sizes_at_the_seams_in_one_call(seams):
    ctxs, xs, b = seams
    sizes = [c.graph.n_nodes for c in ctxs]
    assert set(SEAM_SIZES) <= set(sizes)
    off = b.result_offsets()
    assert off.dtype == np.uint64 and np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    positions, orders, ms = b.results()
    print("read-out of", len(ctxs), "items,", int(off[-1]), "nodes: kernel_ms", ms)
    assert ms > 0.0
    _check_against_contexts(ctxs, xs, positions, orders)
    x_nan = xs[sizes.index(1000)]
    o = orders[sizes.index(1000)]
    nan_at = np.flatnonzero(np.isnan(x_nan))
    assert len(nan_at) == 3 and np.array_equal(o[-3:], nan_at)         # NaNs last, by dense index


def test_per_item_path_above_the_cap(seams):
    ctxs, xs, b = seams
    positions, orders, _ = b.results()
    b.debug_sort_cap(64)
    try:
        positions_64, orders_64, _ = b.results()
    finally:
        b.debug_sort_cap(0)
    for i in range(len(ctxs)):
        assert np.array_equal(positions[i].view(np.uint64), positions_64[i].view(np.uint64)), i
        assert np.array_equal(orders[i], orders_64[i]), i
    _check_against_contexts(ctxs, xs, positions_64, orders_64)
    with pytest.raises(hip.GfsError) as ei:
        b.debug_sort_cap(hip.SEGMENT_SORT_CAP + 1)
    assert ei.value.code == E_ARG
    again = b.results()
    assert all(np.array_equal(a, c) for a, c in zip(again[1], orders))  # (the refused cap changed nothing)


@functools.lru_cache(maxsize=None)
def _oracle_one_stream(name, iter_max):
    """Positions of the oracle's single stream; computed once, never written to."""
    g = load(name)
    og = oracle_graph(g)
    x = O.init_positions(og)
    rc, st, _ = O.sgd_1d(og, oracle_params(_ygs(g, iter_max)), x, n_streams=1)
    assert rc == 0
    x.setflags(write=False)
    return x


def _fixture_ctxs(init):
    ctxs = []
    for name, iter_max in FIXTURES:
        g = load(name)
        ctx, rc = _ctx(g, _ygs(g, iter_max), n_streams=1)
        assert rc == hip.OK
        if init:
            ctx.init_positions()
        ctxs.append(ctx)
    return ctxs


def test_init_run_and_read_out_of_the_fixtures():
    fresh = _fixture_ctxs(init=True)
    ctxs = _fixture_ctxs(init=False)
    for c in ctxs:
        c.upload(np.full(c.graph.n_nodes, -1.0))                       # (whatever was there is overwritten)
    b = hip.Batch(ctxs)
    b.init_positions()
    for c, f in zip(ctxs, fresh):
        assert np.array_equal(c.download().view(np.uint64), f.download().view(np.uint64)), c.graph.n_nodes
    b.run()
    positions, orders, _ = b.results()
    for i, (name, iter_max) in enumerate(FIXTURES):
        x_ref = _oracle_one_stream(name, iter_max)
        assert np.array_equal(positions[i].view(np.uint64), x_ref.view(np.uint64)), name
        assert np.array_equal(orders[i], hip.sort_order(x_ref)), name
    positions_2, orders_2, _ = b.results()                              # a second read-out: the same arrays
    for i in range(len(ctxs)):
        assert np.array_equal(positions[i].view(np.uint64), positions_2[i].view(np.uint64)) and np.array_equal(orders[i], orders_2[i])
    # a read-out between two runs leaves the second run's bits alone
    b.run()
    plain = _fixture_ctxs(init=True)
    pb = hip.Batch(plain)
    pb.run()
    pb.run()
    for c, q in zip(ctxs, plain):
        assert np.array_equal(c.download().view(np.uint64), q.download().view(np.uint64))
        sc, sq = c.stats(), q.stats()
        assert (sc.term_updates, sc.attempts, sc.iterations, sc.launches) == (sq.term_updates, sq.attempts, sq.iterations, sq.launches)
    b.close()
    pb.close()


def test_refusals():
    g = load("simple.gfa")
    lay = []
    for seed in (1, 2):
        c = hip.Context(g)
        lp = P.LayoutSGDParams.from_graph(g, 2, 1)
        lp.seed = seed
        assert c.setup_nd(lp, hip.make_config(n_streams=1)) == hip.OK
        lay.append(c)
    lb = hip.Batch(lay)
    with pytest.raises(hip.GfsError) as ei:
        lb.init_positions()
    assert ei.value.code == E_UNSUPPORTED
    with pytest.raises(hip.GfsError) as ei:
        lb.results()
    assert ei.value.code == E_UNSUPPORTED
    lb.close()
    ctxs = _fixture_ctxs(init=True)
    b = hip.Batch(ctxs)
    total = sum(c.graph.n_nodes for c in ctxs)
    x = np.zeros(total + 1)
    o = np.zeros(total + 1, dtype=np.uint32)
    L = hip.lib()
    for wrong in (total - 1, total + 1, 0):
        assert L.gfs_batch_results(b._h, x.ctypes.data, o.ctypes.data, wrong, None, None) == E_ARG
    assert L.gfs_batch_results(b._h, None, None, total, None, None) == E_ARG
    off = np.zeros(len(ctxs) + 1, dtype=np.uint64)
    assert L.gfs_batch_result_offsets(b._h, off.ctypes.data, len(ctxs)) == E_ARG
    both = b.results()
    only_order = b.results(positions=False)
    only_positions = b.results(order=False)
    assert only_order[0] is None and only_positions[1] is None
    for i, c in enumerate(ctxs):
        assert np.array_equal(only_order[1][i], both[1][i]) and np.array_equal(both[1][i], hip.sort_order(c.download()))
        assert np.array_equal(only_positions[0][i].view(np.uint64), c.download().view(np.uint64))
    b.close()


def test_one_call_is_faster_than_the_per_item_loop():
    """64 DRB1 items after a short run: one results() call against 64 x (download() + sort_order()), each side timed once after
    an untimed call of each.  A condition, not a tuned number: the loop makes 64 x (2 allocations + radix passes + 2 synchronises)."""
    g = load("DRB1-3123.gfa")
    ctxs = []
    for i in range(64):
        ctx, rc = _ctx(g, _ygs(g, 2, seed=9399220 + 1000 * i))
        assert rc == hip.OK
        ctxs.append(ctx)
    b = hip.Batch(ctxs)
    b.init_positions()
    b.run()
    b.results()                                                         # untimed: loads the code object, allocates the scratch
    ctxs[0].download(), ctxs[0].sort_order()
    t0 = time.perf_counter()
    positions, orders, ms = b.results()
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    loop = [(c.download(), c.sort_order()) for c in ctxs]
    t_loop = time.perf_counter() - t0
    print("64 DRB1 items: one results() %.3f ms (kernel_ms %.3f), loop of download + sort_order %.3f ms" % (t_batch * 1e3, ms, t_loop * 1e3))
    for i, (x, o) in enumerate(loop):
        assert np.array_equal(positions[i].view(np.uint64), x.view(np.uint64)) and np.array_equal(orders[i], o), i
    assert len({p.tobytes() for p in positions}) == 64                  # (64 different runs)
    assert t_batch < t_loop, (t_batch, t_loop)
    b.close()


def test_python_batch_sort_reads_through_the_batch():
    from gfasort_amd import sgd as S
    graphs = [load(name) for name, _ in FIXTURES]
    params = [_ygs(g, k) for g, (_, k) in zip(graphs, FIXTURES)]
    out, bs = S.path_sgd_sort_batch(graphs, params, cfg=hip.make_config(n_streams=1))
    assert bs.launches == 1 and bs.items_run == 3
    for res, g in zip(out, graphs):
        assert res["batched"] and res["stats"].launches == 1
        assert res["positions"].shape == (g.n_nodes,) and res["order"].dtype == np.uint64
        assert np.array_equal(res["order"], hip.sort_order(res["positions"]))
