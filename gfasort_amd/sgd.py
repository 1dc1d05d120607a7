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
    per_graph = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * len(graphs)
    params, cfgs = per_graph(params), per_graph(cfg)
    if len(params) != len(graphs) or len(cfgs) != len(graphs):
        raise ValueError("params / cfg: one for all graphs or one per graph")
    result = lambda ctx, batched: dict(positions=ctx.download(), order=ctx.sort_order(), stats=ctx.stats(), batched=batched)
    out = [None] * len(graphs)
    held = {}                                                  # graph index -> its Context, for the batch's candidates
    try:
        for i, (g, p, c) in enumerate(zip(graphs, params, cfgs)):
            out[i] = dict(positions=np.zeros(0), order=np.zeros(0, dtype=np.uint64), stats=None, batched=False)
            if g.n_nodes == 0:
                continue
            ctx = hip.Context(g, device=device)
            try:
                rc = ctx.setup_1d(p, c)
                if rc != hip.OK:                               # nothing to do
                    out[i]["stats"] = ctx.stats()
                    continue
                if ctx.stats().bundle == 1:                    # a candidate: initialised with the batch (or before its solo run)
                    held[i], ctx = ctx, None
                    continue
                ctx.init_positions()
                ctx.run()
                out[i] = result(ctx, False)
            finally:
                if ctx is not None:
                    ctx.close()
        batched, batch, batch_stats = sorted(held), None, None
        while batched and batch is None:
            try:
                batch = hip.Batch([held[i] for i in batched], max_blocks_per_launch)
            except hip.GfsError as e:
                named = re.search(r"batch item (\d+)", str(e))
                if e.code != -5 or not named:                  # GFS_E_UNSUPPORTED names the item: that one runs alone
                    raise
                del batched[int(named.group(1))]
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
        for i, ctx in held.items():
            if i not in batched:
                ctx.init_positions()
                ctx.run()
                out[i] = result(ctx, False)
        return out, batch_stats
    finally:
        for ctx in held.values():
            ctx.close()


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
    per_graph = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * len(graphs)
    params, cfgs = per_graph(params), per_graph(cfg)
    inits = [None] * len(graphs) if inits is None else list(inits)
    if len(params) != len(graphs) or len(cfgs) != len(graphs) or len(inits) != len(graphs):
        raise ValueError("params / cfg / inits: one for all graphs or one per graph")
    out = [None] * len(graphs)

    def alone(i):
        lay, st = path_linear_sgd_layout(graphs[i], params[i], inits[i], cfgs[i], return_stats=True)
        out[i] = dict(layout=lay, stats=st, batched=False)

    held = {}                                                  # graph index -> its Context, for the batches' candidates
    try:
        for i, (g, p, c) in enumerate(zip(graphs, params, cfgs)):
            if g.n_nodes == 0 or p.dimensions not in (2, 3):
                alone(i)
                continue
            ctx = hip.Context(g, device=device)
            try:
                rc = ctx.setup_nd(p, c)
                if rc == hip.OK and ctx.stats().bundle == 1:
                    held[i], ctx = ctx, None
            finally:
                if ctx is not None:
                    ctx.close()                                # nothing to do, or a team-kernel graph: the single call's business
            if i not in held:
                alone(i)
        batch_stats = {}
        for D in (2, 3):
            batched, batch = sorted(i for i in held if params[i].dimensions == D), None
            while batched and batch is None:
                try:
                    batch = hip.Batch([held[i] for i in batched], max_blocks_per_launch)
                except hip.GfsError as e:
                    named = re.search(r"batch item (\d+)", str(e))
                    if e.code != -5 or not named:              # GFS_E_UNSUPPORTED names the item: that one runs alone
                        raise
                    refused = batched.pop(int(named.group(1)))
                    held.pop(refused).close()
                    alone(refused)
            if batch is None:
                continue
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
        return out, batch_stats
    finally:
        for ctx in held.values():
            ctx.close()
