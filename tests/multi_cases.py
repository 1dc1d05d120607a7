"""The inputs of the exact multi-rank merge tests, in one place: tests/test_gpu_multi_merge.py runs them on the GPU,
tests/test_multi_restatement_host.py asserts on the CPU that each of them reaches the edges it is there for.

Every case runs about eleven iterations at one reference stream per rank, with `min_term_updates` set so that no rank
makes more than 40 000 sequential updates.  `iter_max` is 10 unless the annealed rule needs another schedule to reach a
window whose divisor c * cscale lies strictly between 1 and c (at 10 the windows of 3 and 4 iterations jump from
cscale = 1 straight to c * cscale < 1 on these graphs)."""
import functools
from collections import namedtuple

import util
from util import G, P, load
from quality_restatement import noisy_start
from multi_restatement import Cluster, windows_of

ITER_MAX = 10

Case = namedtuple("Case", "id graph world dims merge f64 merge_every sharding whole_vector start updates iter_max steps tags")


def _case(id, graph, world, merge="anneal", f64=False, merge_every=1, dims=0, sharding="auto", whole_vector=False, start="ref",
          updates=6000, iter_max=ITER_MAX, steps=None, tags=()):
    tags = set(tags)
    if merge == "anneal":
        tags.add("anneal")
    if not f64:
        tags.add("f32")
    if dims:
        tags.add("nd")
    return Case(id, graph, world, dims, merge, f64, merge_every, sharding, whole_vector, start, updates, iter_max, steps, frozenset(tags))


def _cases():
    out = []
    # A: a window graph, neighbouring ranks' spans overlap in part.  W = 3 in consecutive blocks of paths has two shared
    # segments ("auto" would interleave 16 equal paths over 3 ranks, and every span would cover the graph).
    for world in (2, 3):
        for merge in ("anneal", "sum", "mean", "touch"):
            for f64 in (False, True):
                for every in (1, 3):
                    out.append(_case(f"A-w{world}-{merge}-{'f64' if f64 else 'f32'}-e{every}", "windows", world, merge, f64, every,
                                     iter_max=12 if every == 3 else ITER_MAX, start="noisy" if every == 3 else "ref",
                                     sharding="contiguous" if world == 3 else "auto", tags=("partial",) if world == 3 else ()))
    out.append(_case("A-w4-whole-anneal-f32-e3", "windows", 4, "anneal", False, 3, whole_vector=True, updates=8000, iter_max=12))
    # B: every path spans the graph: all slots are shared, three ranks move the same nodes
    out.append(_case("B-w3-anneal-f32", "bubbles", 3, "anneal", False, 1, tags=("all3",)))
    out.append(_case("B-w3-touch-f32", "bubbles", 3, "touch", False, 1, start="noisy", tags=("all3",)))
    # C: disjoint spans, an idle rank, nodes no path visits.  The spans share nothing, so the whole vector is exchanged
    # (the last of the three exchanges nothing at all: the windows are empty and only the finish has work)
    out.append(_case("C-w5-lpt-whole-touch-f32", "single_step_shard", 5, "touch", False, 1, sharding="lpt", whole_vector=True,
                     start="noisy", updates=1600, tags=("idle",)))
    out.append(_case("C-w2-whole-mean-f64", "single_step_shard", 2, "mean", True, 3, whole_vector=True, start="noisy", updates=1600))
    out.append(_case("C-w5-lpt-nothing-shared", "single_step_shard", 5, "anneal", False, 1, sharding="lpt", start="noisy", updates=1600,
                     tags=("empty",)))
    # D: layouts
    out.append(_case("D-windows-d2-w3-anneal-f32", "windows", 3, "anneal", False, 2, dims=2, sharding="contiguous", start="gauss",
                     iter_max=8, tags=("partial",)))
    out.append(_case("D-windows-d3-w2-sum-f64", "windows", 2, "sum", True, 2, dims=3, start="gauss"))
    out.append(_case("D-reverse-d2-w3-anneal-f32", "reverse", 3, "anneal", False, 2, dims=2, start="gauss"))
    out.append(_case("D-absent-d3-w2-whole-sum-f64", "absent", 2, "sum", True, 2, dims=3, whole_vector=True, start="gauss", updates=400))
    # E: a real graph with the defaults
    out.append(_case("E-drb1-w2-defaults", "drb1", 2, iter_max=8))
    # F: continuation over a finish, and positions set twice
    out.append(_case("F-continue-w3-anneal-f32-e3", "windows", 3, "anneal", False, 3, sharding="contiguous", start="twice", iter_max=12,
                     steps=(("run", (0, 6)), ("finish",), ("run", (6, 13)), ("finish",)), tags=("partial",)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# G: gfs_rank_run itself, one thread per rank (its windows are the library's own)
RUN_CASE = _case("G-run-w3-anneal-f32-e4", "drb1", 3, "anneal", False, 4)
ALL_CASES = CASES + [RUN_CASE]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "windows":
        return G.synth_windows(6000, 16, 1200, 5)
    if name == "bubbles":
        return G.synth_bubbles(1500, 6, 5)
    if name == "single_step_shard":
        from test_distributed_gloo import _graph
        return _graph("single_step_shard")
    if name == "absent":
        return util.absent_node_graph()
    if name == "reverse":
        return util.reverse_short_paths_graph()
    if name == "drb1":
        return load("DRB1-3123.gfa")
    raise KeyError(name)


def params(case):
    g = graph(case.graph)
    p = P.LayoutSGDParams.from_graph(g, case.dims, 1) if case.dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = case.iter_max
    p.min_term_updates = case.updates
    return p


def starts(case):
    """The arrays set_positions is called with, in order (None: the reference's 1D start)."""
    g = graph(case.graph)
    if case.start == "ref":
        return [None]
    if case.start == "noisy":
        return [noisy_start(g, case.dims, 11)]
    if case.start == "gauss":
        return [util.gaussian_init(g, case.dims, 7)]
    if case.start == "twice":
        return [noisy_start(g, case.dims, 12), None]
    raise KeyError(case.start)


def schedule(case):
    """("window", ks) and ("finish",) steps."""
    steps = case.steps or (("run", (0, case.iter_max + 1)), ("finish",))
    out = []
    for st in steps:
        if st[0] == "run":
            out += [("window", ks) for ks in windows_of(range(*st[1]), case.merge_every, case.iter_max)]
        else:
            out.append(("finish",))
    return out


def cluster(case):
    return Cluster(graph(case.graph), params(case), case.world, dims=case.dims, merge=case.merge, payload_f64=case.f64,
                   sharding=case.sharding, whole_vector=case.whole_vector)


@functools.lru_cache(maxsize=None)
def restated(case_id):
    """The case run through the restatement, once per process; nobody changes what it recorded."""
    case = BY_ID.get(case_id) or RUN_CASE
    cl = cluster(case)
    for x in starts(case):
        cl.set_positions(x)
    for st in schedule(case):
        cl.window(st[1]) if st[0] == "window" else cl.finish()
    for rec in cl.windows:
        for a in rec["moves"] + rec["bufs"] + rec["x"] + [rec["sum"]]:
            a.setflags(write=False)
    for rec in cl.finishes:
        for a in rec["masked"] + [rec["x"]]:
            a.setflags(write=False)
    return cl
