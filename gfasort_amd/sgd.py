"""Host-side mirror of the reference's SGD entry points, running on the HIP engine.

Reference call chain (src/ygs.rs:195-206 -> src/sgd.rs:641-672 -> src/sgd.rs:237-614):
    sgd_sort_only -> path_sgd_sort -> path_linear_sgd
and the layout arm (src/bin/gfasort.rs:265-274 -> src/sgd.rs:773-1188).
Same names, argument meaning and empty-result behaviour; positions are indexed by the dense
node index (position in node_order) exactly like the reference's HashMap<usize,f64> keys.
"""
import re
from typing import Optional, Tuple

import numpy as np

from . import hip
from .graph import FlatGraph
from .layout import Layout
from .params import LayoutSGDParams, PathSGDParams


def path_linear_sgd(graph: FlatGraph, params: PathSGDParams, cfg=None,
                    return_stats: bool = False):
    """sgd.rs:237.  Returns float64[n_nodes] positions, or an EMPTY array when the reference
    returns an empty map (no nodes / no path with more than one step, sgd.rs:242-244,258-261)."""
    if graph.n_nodes == 0:
        return (np.zeros(0), None) if return_stats else np.zeros(0)
    rc, x, st = hip.path_linear_sgd_raw(graph, params, cfg=cfg)
    if rc == hip.NOTHING_TO_DO:
        x = np.zeros(0)
    return (x, st) if return_stats else x


def path_sgd_sort(graph: FlatGraph, params: PathSGDParams, cfg=None) -> np.ndarray:
    """sgd.rs:641-672: dense node indices in ascending position order.  (The reference breaks
    ties by HashMap iteration order, i.e. randomly; here ties keep node_order.)"""
    if graph.n_nodes == 0:
        return np.zeros(0, dtype=np.uint64)
    rc, x, order, st = hip.path_sgd_sort_raw(graph, params, cfg=cfg)       # SGD + device radix sort
    if rc == hip.NOTHING_TO_DO:
        return np.zeros(0, dtype=np.uint64)
    return order


def sgd_sort_only(graph: FlatGraph, params: PathSGDParams, verbose: int = 0, cfg=None) -> np.ndarray:
    """ygs.rs:195-206.  Returns the ordering that `apply_ordering` would consume (empty = the
    reference's no-op, graph_ops.rs:1940)."""
    return path_sgd_sort(graph, params, cfg)


def default_layout_init(graph: FlatGraph, dims: int, seed: int) -> np.ndarray:
    """Initial coordinates in Layout order, as the reference draws them (sgd.rs:829-853): dimension 0 = bp prefix
    (+ end) / prefix + length (- end); dimensions >= 1 = StandardNormal * sqrt(2N) from ONE Xoshiro256+ seeded `seed`,
    node by node.  gfs_init_layout restates rand_distr's ziggurat from its published algorithm: parity unpinned
    (DESIGN.md §5)."""
    return hip.init_layout(graph, dims, seed)


def path_linear_sgd_layout(graph: FlatGraph, params: LayoutSGDParams, init: Optional[np.ndarray] = None,
                           cfg=None, return_stats: bool = False):
    """sgd.rs:773.  Returns a Layout; all-zero when the reference returns `Layout::new`
    (sgd.rs:780-782,795-798)."""
    D = params.dimensions
    if graph.n_nodes == 0:
        lay = Layout(D, 0)
        return (lay, None) if return_stats else lay
    if init is None:
        init = default_layout_init(graph, D, params.seed)
    rc, coords, st = hip.path_linear_sgd_layout_raw(graph, params, init, cfg=cfg)
    lay = Layout(D, graph.n_nodes, coords if rc == hip.OK else None)
    return (lay, st) if return_stats else lay


def _per_graph(v, n):
    """One value for all n graphs, or one per graph: the list."""
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


def _refused_item(e):
    """Which of the contexts handed to hip.Batch its refusal names: GFS_E_UNSUPPORTED's text says which.  Any other code, or a
    text that names no item, is the library's error as it stands."""
    named = re.search(r"batch item (\d+)", str(e))
    if e.code != -5 or not named:
        raise e
    return int(named.group(1))


SET_MAX_NODES = 16384          # graphs of fewer nodes are a batch's candidates under the default policy: created through one ContextSet


def _open_set(graphs, params, cfgs, wanted, device, layouts):
    """One hip.ContextSet for the graphs a batch can take — wanted(i), fewer than SET_MAX_NODES nodes, and a cfg that asks for
    bundle 0 (auto) or 1 — so that their contexts cost one build, not one each, and one set setup (ContextSet.setup_1d, or
    setup_nd for layouts), not one setup each.  Returns (the set or None, {graph index: its Context}, {graph index: what its
    setup returned}); the caller closes the set after everything made from its contexts."""
    def bundle(c):
        return ((int(c.flags) >> 16) & 0xFF) if c is not None else 0
    idx = [i for i, g in enumerate(graphs) if wanted(i) and 0 < g.n_nodes < SET_MAX_NODES and bundle(cfgs[i]) in (0, 1)]
    if not idx:
        return None, {}, {}
    cset = hip.ContextSet([graphs[i] for i in idx], device=device)
    try:
        rcs = (cset.setup_nd if layouts else cset.setup_1d)([params[i] for i in idx], [cfgs[i] for i in idx])
    except Exception:
        cset.close()
        raise
    return cset, dict(zip(idx, cset.contexts)), dict(zip(idx, rcs))


def _batch_of(held, candidates, max_blocks_per_launch):
    """One hip.Batch of the contexts held[i], i in candidates.  A graph the batch refuses moves to the refused ones, for the
    caller to run alone once the batch has run and is closed, and the others are tried again.  Returns (batch, or None when
    nothing is left; the indices in it, in item order; the refused indices)."""
    kept, refused = list(candidates), []
    while kept:
        try:
            return hip.Batch([held[i] for i in kept], max_blocks_per_launch), kept, refused
        except hip.GfsError as e:
            refused.append(kept.pop(_refused_item(e)))
    return None, kept, refused


def path_sgd_sort_batch(graphs, params, cfg=None, max_blocks_per_launch: int = 0, device: int = 0):
    """path_sgd_sort over MANY graphs: the ones whose plan is the fused reference-stream kernel (graphs of fewer than 16384
    nodes under the default policy) run together as one hip.Batch — one persistent launch, or as few as fit the device, with
    their start positions set by one launch before it and their positions and orders read by one Batch.results() after it —
    and the others alone, one after the other.  A graph the batch refuses (hip.Batch names it) is taken out and runs alone;
    the rest still run together.  Only the batch's graphs are resident at once: a graph that runs alone for its bundle is run,
    read back and closed before the next one is set up.  params: one PathSGDParams for all, or one per graph; cfg likewise (or
    None).  Returns one dict per graph, in order: positions (float64[n_nodes]; empty where the reference returns an empty map),
    order (uint64 dense indices in ascending position order; empty likewise), stats (hip.Stats of the graph's context, None for
    an empty graph) and batched (whether it ran in the batch); and the batch's hip.BatchStats (None when nothing was batched)."""
    graphs = list(graphs)
    params, cfgs = _per_graph(params, len(graphs)), _per_graph(cfg, len(graphs))
    if len(params) != len(graphs) or len(cfgs) != len(graphs):
        raise ValueError("params / cfg: one for all graphs or one per graph")

    def alone(ctx):
        ctx.init_positions()
        ctx.run()
        return dict(positions=ctx.download(), order=ctx.sort_order(), stats=ctx.stats(), batched=False)

    out = [None] * len(graphs)
    held = {}                                                  # graph index -> its Context, for the batch's candidates
    cset, made, set_up = _open_set(graphs, params, cfgs, lambda i: True, device, layouts=False)
    try:
        for i, (g, p, c) in enumerate(zip(graphs, params, cfgs)):
            out[i] = dict(positions=np.zeros(0), order=np.zeros(0, dtype=np.uint64), stats=None, batched=False)
            if g.n_nodes == 0:
                continue
            ctx = made[i] if i in made else hip.Context(g, device=device)
            try:
                rc = set_up[i] if i in set_up else ctx.setup_1d(p, c)     # (a graph that runs alone keeps the single call)
                if rc != hip.OK:                               # nothing to do
                    out[i]["stats"] = ctx.stats()
                elif ctx.stats().bundle == 1:                  # a candidate: initialised with the batch (or before its solo run)
                    held[i], ctx = ctx, None
                else:
                    out[i] = alone(ctx)
            finally:
                if ctx is not None:
                    ctx.close()
        batch, batched, refused = _batch_of(held, sorted(held), max_blocks_per_launch)
        batch_stats = None
        if batch is not None:
            try:
                batch.init_positions()
                batch.run()
                batch_stats = batch.stats()
                xs, orders, _ = batch.results()
            finally:
                batch.close()
            for k, i in enumerate(batched):
                out[i] = dict(positions=xs[k], order=orders[k], stats=held[i].stats(), batched=True)
        for i in refused:
            out[i] = alone(held[i])
        return out, batch_stats
    finally:
        for ctx in held.values():
            ctx.close()
        if cset is not None:
            cset.close()


def path_linear_sgd_layout_batch(graphs, params, inits=None, cfg=None, max_blocks_per_launch: int = 0, device: int = 0):
    """path_linear_sgd_layout over MANY graphs, the twin of path_sgd_sort_batch: the graphs whose plan is the pooled
    reference-stream kernel (stats.bundle == 1) and whose dimension a batch kernel is built for (2 and 3) run together, one
    hip.Batch per dimension — all start coordinates up in one Batch.upload_coords(), one persistent launch (or as few as fit
    the device), all final coordinates down in one Batch.coords() — and the others alone through path_linear_sgd_layout, as
    does a graph the batch refuses (hip.Batch names it).  params: one LayoutSGDParams for all, or one per graph; cfg likewise
    (or None); inits: None, or one start array (Layout order) or None per graph — None draws default_layout_init.  Returns one
    dict per graph, in order: layout (the Layout path_linear_sgd_layout returns), stats (hip.Stats, None for an empty graph)
    and batched; and a dict dimension -> hip.BatchStats of the batches that ran."""
    graphs = list(graphs)
    params, cfgs = _per_graph(params, len(graphs)), _per_graph(cfg, len(graphs))
    inits = [None] * len(graphs) if inits is None else list(inits)
    if len(params) != len(graphs) or len(cfgs) != len(graphs) or len(inits) != len(graphs):
        raise ValueError("params / cfg / inits: one for all graphs or one per graph")
    out = [None] * len(graphs)

    def alone(i):
        lay, st = path_linear_sgd_layout(graphs[i], params[i], inits[i], cfgs[i], return_stats=True)
        out[i] = dict(layout=lay, stats=st, batched=False)

    held = {}                                                  # graph index -> its Context, for the batches' candidates
    cset, made, set_up = _open_set(graphs, params, cfgs, lambda i: params[i].dimensions in (2, 3), device, layouts=True)
    try:
        for i, (g, p, c) in enumerate(zip(graphs, params, cfgs)):
            if g.n_nodes == 0 or p.dimensions not in (2, 3):
                alone(i)
                continue
            ctx = made[i] if i in made else hip.Context(g, device=device)
            try:
                rc = set_up[i] if i in set_up else ctx.setup_nd(p, c)     # (a graph that runs alone keeps the single call)
                if rc == hip.OK and ctx.stats().bundle == 1:
                    held[i], ctx = ctx, None
            finally:
                if ctx is not None:
                    ctx.close()                                # nothing to do, or a team-kernel graph: the single call's business
            if i not in held:
                alone(i)
        batch_stats = {}
        for D in (2, 3):
            batch, batched, refused = _batch_of(held, sorted(i for i in held if params[i].dimensions == D), max_blocks_per_launch)
            if batch is not None:
                try:
                    start = [inits[i] if inits[i] is not None else default_layout_init(graphs[i], D, params[i].seed) for i in batched]
                    batch.upload_coords(start)
                    batch.run()
                    batch_stats[D] = batch.stats()
                    coords, _ = batch.coords()
                finally:
                    batch.close()
                for k, i in enumerate(batched):
                    out[i] = dict(layout=Layout(D, graphs[i].n_nodes, coords[k].copy()), stats=held[i].stats(), batched=True)
            for i in refused:
                held.pop(i).close()                            # (the single call sets its own context up)
                alone(i)
        return out, batch_stats
    finally:
        for ctx in held.values():
            ctx.close()
        if cset is not None:
            cset.close()
