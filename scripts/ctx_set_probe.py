"""Host wall time of creating the contexts of many small graphs: a loop of gfs_ctx_create against one gfs_ctx_set_create (K3b).
Prints every run and the median of 5 after gfs_warmup, with the set's launch count and arena size.

    python scripts/ctx_set_probe.py > profiles/r17/ctx_set_probe.log
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gfasort_amd import graph as G  # noqa: E402
from gfasort_amd import hip  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
RUNS = 5


def loop_ms(graphs):
    t0 = time.perf_counter()
    ctxs = [hip.Context(g) for g in graphs]
    ms = (time.perf_counter() - t0) * 1e3
    for c in ctxs:
        c.close()
    return ms


def set_ms(graphs):
    t0 = time.perf_counter()
    s = hip.ContextSet(graphs)
    ms = (time.perf_counter() - t0) * 1e3
    info = s.info()
    s.close()
    return ms, info


def main():
    hip.check(hip.lib().gfs_warmup(0))
    drb1, simple, lil = (G.load_gfa(os.path.join(DATA, n)) for n in ("DRB1-3123.gfa", "simple.gfa", "lil.gfa"))
    cases = [("64 x DRB1-3123", [drb1] * 64), ("256 x DRB1-3123", [drb1] * 256), ("86 x (simple, lil, DRB1-3123) = 258", [simple, lil, drb1] * 86)]
    loop_ms([drb1] * 4), set_ms([drb1] * 4)                      # (first use of both paths)
    for name, graphs in cases:
        loops, sets, info = [], [], None
        for r in range(RUNS):                                   # interleaved
            loops.append(loop_ms(graphs))
            ms, info = set_ms(graphs)
            sets.append(ms)
            print(f"{name}: run {r}: loop of gfs_ctx_create {loops[-1]:9.2f} ms | gfs_ctx_set_create {sets[-1]:8.2f} ms (build_ms {info.build_ms:.2f})")
        print(f"{name}: median of {RUNS}: loop {statistics.median(loops):.2f} ms [{min(loops):.2f} .. {max(loops):.2f}] | "
              f"set {statistics.median(sets):.2f} ms [{min(sets):.2f} .. {max(sets):.2f}] | "
              f"ratio {statistics.median(loops) / statistics.median(sets):.1f}x | set: launches {info.launches}, "
              f"device_allocations {info.device_allocations}, arena_bytes {info.arena_bytes}, nodes {info.total_nodes}, steps {info.total_steps}")


if __name__ == "__main__":
    main()
