"""CPU side of the exact multi-rank merge tests (tests/test_gpu_multi_merge.py holds the GPU side).

(a) Every input of tests/multi_cases.py reaches the edge it is there for, computed from the restatement alone: a GPU case
    cannot pass because nothing was shared, nothing was touched twice or the divisor never left 1.  These are conditions of
    the inputs; an input that misses one is changed, never the condition.
(b) The restatement against ShardedSGD (gfasort_amd/distributed.py) under gloo at world 2, where a sum of two is order-free:
    final positions equal bit for bit.  With the GPU file this ties the CPU driver, the restatement and the kernels together."""
import os

import numpy as np
import pytest

import multi_cases as MC
from multi_restatement import bits, mean_node_length
from util import O, oracle_graph

IDS = [c.id for c in MC.ALL_CASES]


def _case(cid):
    return MC.BY_ID.get(cid) or MC.RUN_CASE


def _touched(cl):
    """Per window: the summed touched counts, as float64."""
    return [w["sum"][cl.total:].astype(np.float64) for w in cl.windows]


@pytest.mark.parametrize("name", sorted({c.graph for c in MC.ALL_CASES}))
def test_mean_node_length_rounds_alike_both_ways(name):
    """eta_sum: the product divides in long double and rounds once, ShardedSGD divides in float64.  On these graphs both
    give the same double; a graph where they differ has to be named in multi_restatement.py, not hidden."""
    as_product, plain = mean_node_length(MC.graph(name))
    assert as_product == plain


@pytest.mark.parametrize("cid", IDS)
def test_no_rank_runs_more_than_40000_updates(cid):
    cl = MC.restated(cid)
    assert max(cl.quotas) * (_case(cid).iter_max + 1) <= 40_000 and sum(cl.quotas) == _case(cid).updates


@pytest.mark.parametrize("cid", IDS)
def test_moves_of_both_signs_are_exchanged(cid):
    case, cl = _case(cid), MC.restated(cid)
    if "empty" in case.tags:
        # the one case that is there for having nothing to exchange: its windows are empty, its finish is not
        assert cl.total == 0 and cl.segments == [] and all(b.size == 0 for w in cl.windows for b in w["bufs"])
        assert sum(int((m != 0).any()) for m in cl.finishes[-1]["masked"]) >= 2
        assert not np.array_equal(bits(cl.finishes[-1]["x"]), bits(np.ascontiguousarray(MC.starts(case)[-1])))
        return
    assert cl.total > 0
    deltas = np.concatenate([b[:cl.total] for w in cl.windows for b in w["bufs"]])
    assert (deltas < 0).any() and (deltas > 0).any()
    assert len(cl.windows) == len([s for s in MC.schedule(case) if s[0] == "window"]) >= 3
    assert len(cl.windows[-1]["ks"]) < case.merge_every or case.merge_every == 1          # a short last window


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "anneal" in c.tags and "empty" not in c.tags])
def test_anneal_cases_reach_both_regimes_and_the_clamp(cid):
    cl = MC.restated(cid)
    cs = [w["cscale"] for w in cl.windows]
    assert any(v == 1.0 for v in cs) and any(0.0 < v < 1.0 for v in cs)
    t = _touched(cl)
    assert any((v == 1.0).any() for v in t) and any((v >= 2.0).any() for v in t)
    assert any(((v >= 2.0) & (v * w["cscale"] < 1.0)).any() for v, w in zip(t, cl.windows))
    # and the divisor is really c * cscale somewhere: above 1 and not an integer
    assert any((((v * w["cscale"]) > 1.0) & ((v * w["cscale"]) % 1.0 != 0.0)).any() for v, w in zip(t, cl.windows))


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "all3" in c.tags])
def test_whole_graph_cases_have_nodes_all_three_ranks_moved(cid):
    case, cl = _case(cid), MC.restated(cid)
    assert case.world == 3 and any((v == 3.0).any() for v in _touched(cl))
    visited = np.unique(cl.g.step_node[cl.g.step_node != 0xFFFFFFFF]).shape[0]
    assert cl.segments == [(0, visited)]                                        # every slot a path steps on is shared


def test_the_whole_vector_case_exchanges_every_slot():
    cl = MC.restated("A-w4-whole-anneal-f32-e3")
    assert cl.world == 4 and cl.segments == [(0, cl.g.n_nodes)] and cl.total == cl.g.n_nodes
    assert len({r for _, _, r in cl.plan.owned}) == 4


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "f32" in c.tags and "empty" not in c.tags])
def test_f32_cases_round_a_move(cid):
    cl = MC.restated(cid)
    assert cl.T == np.float32
    assert any((m.astype(np.float32).astype(np.float64) != m).any() for w in cl.windows for m in w["moves"])


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "partial" in c.tags])
def test_partial_overlap_cases(cid):
    cl = MC.restated(cid)
    shared = sum(hi - lo for lo, hi in cl.segments)
    assert len(cl.segments) >= 2 and 0 < shared < cl.g.n_nodes
    assert len({r for _, _, r in cl.plan.owned}) >= 2
    assert cl.total == shared * cl.planes


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "idle" in c.tags])
def test_idle_case(cid):
    case, cl = _case(cid), MC.restated(cid)
    assert sum(cl.idle) == 1
    r = cl.idle.index(True)
    assert cl.total > 0 and all(w["bufs"][r].size == 2 * cl.total and not w["bufs"][r].any() for w in cl.windows)
    assert not (cl.finishes[-1]["masked"][r] != 0).any() or r == 0
    covered = np.zeros(cl.g.n_nodes, dtype=bool)
    for lo, hi in zip(cl.plan.span_lo, cl.plan.span_hi):
        covered[int(lo):int(hi)] = True
    gaps = [(lo, hi) for lo, hi, owner in cl.plan.owned if owner == 0 and not covered[lo:hi].any()]
    assert gaps
    x0 = np.ascontiguousarray(MC.starts(case)[-1])
    for lo, hi in gaps:
        nodes = cl.node_of_slot[lo:hi]
        assert np.array_equal(bits(cl.finishes[-1]["x"][nodes]), bits(x0[nodes])) and (x0[nodes] != 0).all()


@pytest.mark.parametrize("cid", [c.id for c in MC.ALL_CASES if "nd" in c.tags])
def test_layout_cases_reach_the_last_plane(cid):
    case, cl = _case(cid), MC.restated(cid)
    assert cl.planes == 2 * case.dims and np.array_equal(np.unique(cl.elem_plane), np.arange(cl.planes))
    lo, hi = cl.segments[-1]
    last = (cl.elem_plane == cl.planes - 1) & (cl.elem_slot >= lo) & (cl.elem_slot < hi)
    assert last.any() and last[-1] and any((b[cl.total:][last] != 0).any() for w in cl.windows for b in w["bufs"])
    # every plane carries moves of its own: no two planes' deltas are the same vector
    per_plane = [np.concatenate([w["sum"][:cl.total][cl.elem_plane == r] for w in cl.windows]) for r in range(cl.planes)]
    assert all(not np.array_equal(per_plane[a], per_plane[b]) for a in range(cl.planes) for b in range(a))


def test_continuation_case_snapshots_again():
    cl = MC.restated("F-continue-w3-anneal-f32-e3")
    assert len(cl.finishes) == 2 and \
        [w["ks"] for w in cl.windows] == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12]]
    # the first finish moved shared elements of some replica (what the re-snapshot must pick up)
    before, after = cl.windows[1]["x"], cl.finishes[0]["x"]
    assert any(not np.array_equal(bits(before[r]), bits(after)) for r in range(cl.world))
    assert len(MC.starts(MC.BY_ID["F-continue-w3-anneal-f32-e3"])) == 2


# ---- (b) the restatement against ShardedSGD under gloo ---------------------------------------------------------------
def _worker(rank, world, port, cid, out):
    import torch
    import torch.distributed as dist
    from gfasort_amd.distributed import ShardedSGD
    from test_distributed_gloo import OracleEngine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    case = MC.BY_ID[cid]
    g, p = MC.graph(case.graph), MC.params(case)
    r = ShardedSGD(g, p, rank, world, OracleEngine, dims=case.dims, streams_per_rank=1, merge=case.merge, dist=dist,
                   merge_every=case.merge_every, sharding=case.sharding, whole_vector=case.whole_vector, payload_f64=case.f64)
    for x in MC.starts(case):
        r.set_positions(O.init_positions(oracle_graph(g)) if x is None else x)
    r.run()
    x = torch.from_numpy(r.positions_numpy())
    gathered = [torch.zeros_like(x) for _ in range(world)]
    dist.all_gather(gathered, x)
    if rank == 0:
        out.put([t.numpy() for t in gathered])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("cid", ["A-w2-anneal-f32-e1", "A-w2-touch-f64-e3"])
def test_restatement_equals_sharded_sgd_under_gloo(cid):
    import torch.multiprocessing as mp
    from test_distributed_gloo import _free_port
    case = MC.BY_ID[cid]
    assert case.world == 2 and case.dims == 0
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, cid, out)) for r in range(2)]
    for pr in procs:
        pr.start()
    xs = out.get(timeout=240)
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    want = MC.restated(cid).finishes[-1]["x"]
    for r in range(2):
        assert np.array_equal(bits(xs[r]), bits(want)), (r, int(np.flatnonzero(bits(xs[r]) != bits(want))[0]))
