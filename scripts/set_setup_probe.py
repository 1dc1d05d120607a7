"""Host wall time of setting up the 256 items of one context set: (a) the loop of gfs_ctx_setup_1d / _nd over the items, which is
what the batch drivers do, against (b) one gfs_ctx_set_setup_1d / _nd (K3c).  256 x DRB1-3123, for the parameters of `-p Y` and of
`-p L --dimensions 2`; one process; every timed setup is the first one of a freshly built set (what a driver's set sees), after one
untimed round of both; prints every run and the median of 5, and the allocations, copies and launches of both — the set's as
gfs_ctx_set_setup_info counts them, the loop's counted from capi.hip setup_common (per item, reference streams: five
allocations — positions, zeta table, RNG words, counters, schedule table — three copies and two memsets).  The last line per case
says whether (b) is below (a) by more than the spread of (a)'s five runs: the rule by which the drivers take the set call.

    python scripts/set_setup_probe.py > profiles/r23/set_setup_probe.log
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gfasort_amd import graph as G  # noqa: E402
from gfasort_amd import hip  # noqa: E402
from gfasort_amd import params as P  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
RUNS, ITEMS = 5, 256
LOOP_PER_ITEM = (5, 3, 2)                              # allocations, copies, launches (memsets) of one gfs_ctx_setup_*: see above


def timed(graphs, setup):
    """setup(set) on a freshly built set: its wall time in ms and the set's setup info."""
    s = hip.ContextSet(graphs)
    try:
        t0 = time.perf_counter()
        setup(s)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, s.setup_info
    finally:
        s.close()


def main():
    hip.check(hip.lib().gfs_warmup(0))
    g = G.load_gfa(os.path.join(DATA, "DRB1-3123.gfa"))
    graphs = [g] * ITEMS
    sort_p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    layout_p = P.LayoutSGDParams.from_graph(g, 2, 1)
    cases = [
        ("-p Y", lambda s: [c.setup_1d(sort_p) for c in s.contexts], lambda s: s.setup_1d(sort_p)),
        ("-p L --dimensions 2", lambda s: [c.setup_nd(layout_p) for c in s.contexts], lambda s: s.setup_nd(layout_p)),
    ]
    for name, loop, one in cases:
        timed(graphs, loop), timed(graphs, one)                # (the untimed round: first use of both paths)
        loops, sets, info = [], [], None
        for r in range(RUNS):                                   # interleaved
            loops.append(timed(graphs, loop)[0])
            ms, info = timed(graphs, one)
            sets.append(ms)
            print(f"{ITEMS} x DRB1-3123, {name}: run {r}: (a) loop of gfs_ctx_setup {loops[-1]:9.2f} ms | (b) gfs_ctx_set_setup {sets[-1]:8.2f} ms "
                  f"(setup_ms {info.setup_ms:.2f})")
        a, b, spread = statistics.median(loops), statistics.median(sets), max(loops) - min(loops)
        print(f"{ITEMS} x DRB1-3123, {name}: median of {RUNS}: (a) {a:.2f} ms [{min(loops):.2f} .. {max(loops):.2f}] | "
              f"(b) {b:.2f} ms [{min(sets):.2f} .. {max(sets):.2f}] | ratio {a / b:.1f}x")
        print(f"{ITEMS} x DRB1-3123, {name}: (a) allocations {ITEMS * LOOP_PER_ITEM[0]}, copies {ITEMS * LOOP_PER_ITEM[1]}, launches {ITEMS * LOOP_PER_ITEM[2]} "
              f"(counted from the code) | (b) allocations {info.device_allocations}, copies {info.copies}, launches {info.launches}, "
              f"streams {info.total_streams}, state_bytes {info.state_bytes}")
        print(f"{ITEMS} x DRB1-3123, {name}: (b) below (a) by more than (a)'s spread of {spread:.2f} ms: {'yes' if b < a - spread else 'no'}")


if __name__ == "__main__":
    main()
