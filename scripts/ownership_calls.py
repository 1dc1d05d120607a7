"""One pass over the entry points that allocate, free, create and destroy: a context's create, setup_1d, init_positions, run,
sort_order, pair_errors and destroy, then a batch of 3 small sorts with run, results(), one call of each batch read-out
(pair_errors, path_errors, stretched_pairs with cap 4, node_errors, sort_quality) and close, then a batch of 3 small 2-D layouts
with upload_coords, coords and pair_errors.  For a trace of the runtime's calls, to compare two builds of the library call for call
(GFS_LIB_PATH selects the build):

    rocprofv3 --hip-trace --stats -d OUT -- python scripts/ownership_calls.py

The per-API counts of hipMalloc, hipFree, hipHostMalloc, hipHostFree, hipEventCreate, hipEventDestroy, hipMemcpy*, hipMemset*
hipLaunchKernel, hipStreamSynchronize and hipDeviceSynchronize of the two runs must be equal (profiles/r15/, profiles/r20/).
Prints a digest of what it computed, equal on both builds.

usage: ownership_calls.py [data_dir]      default: tests/data
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    h = hashlib.sha256()
    g = G.load_gfa(os.path.join(data, "DRB1-3123.gfa"))
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = 5
    ctx = hip.Context(g)
    assert ctx.setup_1d(p, hip.make_config(n_streams=1)) == hip.OK
    ctx.init_positions()
    assert ctx.run() == hip.OK
    h.update(ctx.download().tobytes())
    h.update(ctx.sort_order().tobytes())
    h.update(ctx.pair_errors([1, 2, 10]).tobytes())
    ctx.close()

    ctxs = []
    for name in ("simple.gfa", "lil.gfa", "DRB1-3123.gfa"):
        gi = G.load_gfa(os.path.join(data, name))
        pi = P.YgsParams.from_graph(gi, 0, 1).path_sgd
        pi.iter_max = 5
        c = hip.Context(gi)
        assert c.setup_1d(pi, hip.make_config(n_streams=1)) == hip.OK
        ctxs.append(c)
    b = hip.Batch(ctxs)
    b.init_positions()
    assert b.run() == hip.OK
    xs, orders, _ = b.results()
    for x, o in zip(xs, orders):
        h.update(np.ascontiguousarray(x).tobytes())
        h.update(np.ascontiguousarray(o).tobytes())
    h.update(b.pair_errors([1, 2, 10]).tobytes())
    for rows in b.path_errors(2, 0.5) + b.node_errors(2, 0.5):
        h.update(np.ascontiguousarray(rows).tobytes())
    lists, totals = b.stretched_pairs(2, 0.5, cap=4)
    for rows in lists:
        h.update(np.ascontiguousarray(rows).tobytes())
    h.update(np.ascontiguousarray(totals).tobytes())
    h.update(repr([sorted(q.items()) for q in b.sort_quality()]).encode())
    b.close()
    for c in ctxs:
        c.close()

    ctxs = []
    for name in ("simple.gfa", "lil.gfa", "DRB1-3123.gfa"):
        gi = G.load_gfa(os.path.join(data, name))
        pi = P.LayoutSGDParams.from_graph(gi, 2, 1)
        pi.iter_max = 5
        c = hip.Context(gi)
        assert c.setup_nd(pi, hip.make_config(n_streams=1)) == hip.OK
        ctxs.append(c)
    b = hip.Batch(ctxs)
    rng = np.random.default_rng(5)
    b.upload_coords([rng.normal(0.0, 100.0, c.graph.n_nodes * 4) for c in ctxs])
    for x in b.coords()[0]:
        h.update(np.ascontiguousarray(x).tobytes())
    h.update(b.pair_errors([1, 2, 10]).tobytes())
    b.close()
    for c in ctxs:
        c.close()
    print("library:", hip.lib_path() if not os.environ.get("GFS_LIB_PATH") else os.environ["GFS_LIB_PATH"])
    print("digest:", h.hexdigest())


if __name__ == "__main__":
    main()
