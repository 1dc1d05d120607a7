"""The buffers a context and a batch keep between calls and grow on demand (capi_ctx.h gfs::Buffer: the K7 scratch, the schedule
slice and the pool counters of a context; the packed outputs, the per-item sort's scratch, the pinned staging and the coordinate
and quality buffers of a batch), when calls come in an order the feature tests do not use: a reused buffer that is too small, or
that the next user overwrites, changes a result.  Every comparison is bit for bit, against the same call made once on a fresh
context, or against the per-item calls on the batch's own contexts."""
import numpy as np
import pytest

from util import P, load, gaussian_init
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

FIXTURES = ("simple.gfa", "lil.gfa", "DRB1-3123.gfa")                  # in ascending size
RATIO = 0.5                                                            # nearly every pair counts as stretched: the lists are long


def _ygs(g, iter_max):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    return p


def _bytes(v):
    """A result as bytes: arrays (structured ones too, NaNs and all) by their memory, the rest by repr."""
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if isinstance(v, (tuple, list)):
        return b"|".join(_bytes(e) for e in v)
    if isinstance(v, dict):
        return _bytes([(k, v[k]) for k in sorted(v)])
    if isinstance(v, float):
        return np.float64(v).tobytes()
    return repr(v).encode()


# ---- case 1: one context, the K7 scratch shared by six read-outs -----------------------------------------------------------
def _positions(g, dims):
    """Fixed positions that are no solution: the start plus noise (1D), Box-Muller coordinates (layouts)."""
    if dims == 0:
        return hip.init_positions(g) + np.random.default_rng(3).normal(0.0, 30.0, g.n_nodes)
    return gaussian_init(g, dims, 7)


def _context(g, dims, x):
    ctx = hip.Context(g)
    if dims == 0:
        ctx.setup_1d(_ygs(g, 3), hip.make_config(n_streams=1))
    else:
        p = P.LayoutSGDParams.from_graph(g, dims, 1)
        p.iter_max = 3
        ctx.setup_nd(p, hip.make_config(n_streams=1))
    ctx.upload(x)
    return ctx


@pytest.mark.parametrize("dims", [0, 2])
def test_readouts_share_one_scratch(dims):
    g = load("lil.gfa")
    x = _positions(g, dims)
    above = g.n_steps + 10                                             # a cap above any total
    calls = [
        ("pair_errors 1", lambda c: c.pair_errors([1])),
        ("pair_errors 7", lambda c: c.pair_errors([1, 2, 3, 5, 8, 13, 21])),
        ("path_errors", lambda c: c.path_errors(2, RATIO)),
        ("node_errors", lambda c: c.node_errors(2, RATIO)),
        ("stretched_pairs cap 1", lambda c: c.stretched_pairs(2, RATIO, cap=1)),
        ("stretched_pairs cap above", lambda c: c.stretched_pairs(2, RATIO, cap=above)),
        ("sort_quality", (lambda c: c.sort_quality()) if dims == 0 else None),
        ("stress_of_pairs 3", lambda c: c.stress_of_pairs([0, 5, 10], [3, 9, 20])),
        ("pair_errors 1 again", lambda c: c.pair_errors([1])),
    ]
    calls = [(name, f) for name, f in calls if f is not None]
    ctx = _context(g, dims, x)
    try:
        got = [_bytes(f(ctx)) for _, f in calls]
        total = ctx.stretched_pairs(2, RATIO, cap=0)[1]
    finally:
        ctx.close()
    assert 1 < total < above                                           # the two caps are below and above it
    for (name, f), have in zip(calls, got):
        fresh = _context(g, dims, x)
        try:
            assert _bytes(f(fresh)) == have, name
        finally:
            fresh.close()
    assert got[0] == got[-1]


# ---- case 2: one context, the schedule slice and the pool counters ---------------------------------------------------------
def test_schedule_slice_and_pools_grow_then_serve_shorter_lists():
    """One stream: what the existing tests hold a fused launch and one launch per iteration equal at, bit for bit
    (test_gpu_parity.py test_reference_streams_fused_equal_unfused_equal_oracle_on_one_stream).  Lists that are not consecutive go
    through the context's own slice of the schedule; each launch zeroes its part of the pool counters."""
    g = load("simple.gfa")
    p = _ygs(g, 10)
    lists = ([3, 1], [0, 2, 4, 1, 3], [2, 0, 1])
    out = []
    for fused in (True, False):
        ctx = hip.Context(g)
        try:
            ctx.setup_1d(p, hip.make_config(n_streams=1))
            ctx.init_positions()
            for ks in lists:
                if fused:
                    ctx.run_range(ks)
                else:
                    for k in ks:
                        ctx.run_iteration(k)
            ctx.synchronize()
            st = ctx.stats()
            assert st.iterations == 10 and st.launches == (3 if fused else 10) and st.term_updates == 10 * p.min_term_updates
            out.append(ctx.download())
        finally:
            ctx.close()
    assert np.isfinite(out[0]).all() and not np.array_equal(out[0], hip.init_positions(g))
    assert out[0].tobytes() == out[1].tobytes()


# ---- cases 3 and 4: one batch, its packed outputs, sort scratch, staging, coordinate and quality buffers ----------------------
def _batch(dims):
    ctxs = []
    for name in FIXTURES:
        g = load(name)
        ctx = hip.Context(g)
        if dims == 0:
            ctx.setup_1d(_ygs(g, 5), hip.make_config(n_streams=1))
        else:
            p = P.LayoutSGDParams.from_graph(g, dims, 1)
            p.iter_max = 5
            ctx.setup_nd(p, hip.make_config(n_streams=1))
        ctxs.append(ctx)
    sizes = [c.graph.n_nodes for c in ctxs]
    assert sizes == sorted(sizes) and sizes[0] > 1
    return ctxs, hip.Batch(ctxs)


def _check_pair_errors(b, ctxs, zs):
    rows = b.pair_errors(zs)
    assert rows.shape == (len(ctxs), len(zs))
    for i, c in enumerate(ctxs):
        assert rows[i].tobytes() == c.pair_errors(zs).tobytes(), (i, zs)


def _check_readouts_interleaved(b, ctxs, sorts):
    """Every batch read-out in the order small map, large map, small map, each bit for bit the per-context call: the diagnosis and
    the sort quality share the batch's quality buffer and pinned staging with pair_errors, and the staging with results."""
    above = max(c.graph.n_steps for c in ctxs) + 10                      # a cap above every total

    def path_errors():
        for i, rows in enumerate(b.path_errors(2, RATIO)):
            assert _bytes(rows) == _bytes(ctxs[i].path_errors(2, RATIO)), i

    def stretched_pairs(cap):
        lists, totals = b.stretched_pairs(2, RATIO, cap=cap)
        for i, c in enumerate(ctxs):
            rows, total = c.stretched_pairs(2, RATIO, cap=cap)
            assert int(totals[i]) == int(total) and _bytes(lists[i]) == _bytes(rows), (i, cap)

    def node_errors():
        for i, rows in enumerate(b.node_errors(2, RATIO)):
            assert _bytes(rows) == _bytes(ctxs[i].node_errors(2, RATIO)), i

    def sort_quality():
        for i, q in enumerate(b.sort_quality()):
            assert _bytes(q) == _bytes(ctxs[i].sort_quality()), i

    def results():
        xs, orders, _ = b.results()
        for i, c in enumerate(ctxs):
            assert np.array_equal(orders[i], c.sort_order()) and xs[i].tobytes() == c.download().tobytes(), i

    calls = [path_errors, lambda: stretched_pairs(1), lambda: stretched_pairs(above), node_errors] + ([sort_quality] if sorts else []) + \
            [lambda: _check_pair_errors(b, ctxs, [1, 2, 3, 10, 100])] + ([results] if sorts else [])
    small, large = lambda: _check_pair_errors(b, ctxs, [1]), lambda: stretched_pairs(above)
    for call in calls:
        small()
        large()
        call()
        small()
    totals = b.stretched_pairs(2, RATIO, cap=0)[1]
    assert max(int(t) for t in totals) > 1 and all(int(t) < above for t in totals)   # cap 1 cuts a list short, the other none


def test_batch_of_sorts_reuses_its_buffers():
    ctxs, b = _batch(0)

    def check_results(positions):
        xs, orders, _ = b.results(positions=positions)
        for i, c in enumerate(ctxs):
            assert np.array_equal(orders[i], c.sort_order()), i
            if positions:
                assert xs[i].tobytes() == c.download().tobytes(), i
    try:
        _check_pair_errors(b, ctxs, [1])                               # small staging (positions still zero)
        b.init_positions()
        assert b.run() == hip.OK
        check_results(False)
        check_results(True)                                            # the staging grows
        b.debug_sort_cap(ctxs[0].graph.n_nodes - 1)                    # every item takes the per-item sort, smallest first
        check_results(True)
        _check_pair_errors(b, ctxs, [1, 2, 3, 10, 100])
        assert not any(np.array_equal(c.download(), hip.init_positions(c.graph)) for c in ctxs)   # (the run moved every item)
        b.debug_sort_cap(0)                                            # the default sort cap, then every item above it again
        _check_readouts_interleaved(b, ctxs, True)
        b.debug_sort_cap(ctxs[0].graph.n_nodes - 1)
        _check_readouts_interleaved(b, ctxs, True)
    finally:
        b.close()
        for c in ctxs:
            c.close()


def test_batch_of_layouts_reuses_its_buffers():
    ctxs, b = _batch(2)
    up = [gaussian_init(c.graph, 2, 11 + i) for i, c in enumerate(ctxs)]
    try:
        _check_pair_errors(b, ctxs, [1])
        b.upload_coords(up)
        for i, x in enumerate(b.coords()[0]):
            assert x.tobytes() == up[i].tobytes(), i
        _check_pair_errors(b, ctxs, [1, 2, 3, 10, 100])
        for i, x in enumerate(b.coords()[0]):
            assert x.tobytes() == up[i].tobytes(), i
        for i, c in enumerate(ctxs):
            assert c.download().tobytes() == up[i].tobytes(), i         # (what the batch uploaded is what the item holds)
        _check_readouts_interleaved(b, ctxs, False)
    finally:
        b.close()
        for c in ctxs:
            c.close()
