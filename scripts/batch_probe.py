"""What does a batch (gfs_batch, K1f: sgd_kernels_batch.hip) buy?  N graphs in one persistent launch against the same N graphs
one after the other, each in its own fused launch (K1d, unchanged).

For N = 1, 8, 64, 256 items of DRB1-3123 with distinct seeds at the -p Y defaults, and for a mixed list that repeats simple, lil
and DRB1: the batch's kernel ms (HIP events around its launches; median of 3 runs after one untimed run), its launches and
workgroups, the sum of the items' solo kernel ms, and the ratio of the two.  Then the smallest N of DRB1 items at which the batch
needs two launches (found by running batches; their times are not used).

usage: batch_probe.py [data_dir]      default: tests/data
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip


def make(g, seed):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.seed = seed
    ctx = hip.Context(g)
    assert ctx.setup_1d(p) == hip.OK
    ctx.init_positions()
    return ctx


def restart(ctxs):
    for c in ctxs:
        c.reset_streams()
        c.init_positions()


def measure(label, ctxs):
    b = hip.Batch(ctxs)
    b.run()                                                    # untimed: loads the code object, sizes nothing else
    times = []
    for _ in range(3):
        restart(ctxs)
        before = b.stats()
        b.run()
        after = b.stats()
        times.append(after.kernel_ms - before.kernel_ms)
    launches, blocks = after.launches - before.launches, after.blocks - before.blocks
    updates = after.term_updates                               # (the counters were reset with the streams)
    b.close()
    solo, slowest = 0.0, 0.0
    for c in ctxs:
        c.reset_streams()
        c.init_positions()
        c.run()
        ms = c.stats().kernel_ms
        solo += ms
        slowest = max(slowest, ms)
    t = float(np.median(times))
    print(f"{label}: batch kernels {t:.3f} ms (runs: {' '.join('%.3f' % v for v in times)}), {launches} launch(es), {blocks} workgroups, "
          f"{updates} updates = {updates / (t * 1e-3) / 1e9:.2f} G updates/s | solo: sum {solo:.3f} ms, slowest item {slowest:.3f} ms | "
          f"batch / sum of solo = {t / solo:.4f}, batch / slowest = {t / slowest:.2f}", flush=True)


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    drb1, simple, lil = (G.load_gfa(os.path.join(data, n)) for n in ("DRB1-3123.gfa", "simple.gfa", "lil.gfa"))
    try:
        import torch
        props = torch.cuda.get_device_properties(0)
        print(f"device: {props.name}, {props.multi_processor_count} CUs")
    except Exception as e:                                     # (the probe itself needs no torch)
        print(f"device: not asked ({e})")
    print(f"DRB1-3123: {drb1.n_nodes} nodes, {drb1.n_steps} steps; simple: {simple.n_nodes} nodes; lil: {lil.n_nodes} nodes")
    pool = [make(drb1, 9399220 + 1000 * i) for i in range(256)]
    st = pool[0].stats()
    print(f"a DRB1 item: {st.n_streams} streams = {(st.n_streams + 255) // 256} workgroups of 256, bundle {st.bundle}")
    for n in (1, 8, 64, 256):
        measure(f"DRB1 x {n}", pool[:n])
    for n in (9, 66, 258):
        mixed = [make((simple, lil, drb1)[i % 3], 9399220 + 7 * i) for i in range(n)]
        measure(f"simple, lil, DRB1 repeated to {n}", mixed)
        for c in mixed:
            c.close()
    # the first N that needs two launches: bisect on the number of launches a batch of the first N items makes
    pool += [make(drb1, 9399220 + 1000 * i) for i in range(256, 1024)]

    def launches(n):
        b = hip.Batch(pool[:n])
        b.run()
        k = b.stats().launches
        b.close()
        return k
    if launches(len(pool)) == 1:
        print(f"{len(pool)} DRB1 items still fit one launch")
    else:
        lo, hi = 1, len(pool)                                  # launches(lo) == 1 < launches(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if launches(mid) == 1 else (lo, mid)
        per_item = (st.n_streams + 255) // 256
        print(f"DRB1 items: {lo} fit one launch ({lo * per_item} workgroups), {hi} need two: one launch holds fewer than "
              f"{hi * per_item} workgroups")
    for c in pool:
        c.close()


if __name__ == "__main__":
    main()
