"""What does the batched sort quality (gfs_batch_sort_quality, K7k: batch_sort_quality_kernels.hip) buy?

For N = 64 and 256 items of DRB1-3123 with distinct seeds, set up as 1D sorts at the `-p Y` defaults and run once as a batch, host
wall time (time.perf_counter) of
  * N x Context.sort_quality()   — the only way a batch had before it had its own — against
  * one Batch.sort_quality(), and its kernel_ms,
the two interleaved in one process: one untimed call of each, then five rounds of (loop, batch); every run and the medians.
Before timing, the batch's rows are compared with the loop's (equal, or the probe stops).

usage: batch_sort_quality_probe.py [data_dir]      default: tests/data
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip


def timed_ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    drb1 = G.load_gfa(os.path.join(data, "DRB1-3123.gfa"))
    print(f"DRB1-3123: {drb1.n_nodes} nodes (padded 8192), {drb1.n_steps} steps, {-(-drb1.n_steps // 2048)} workgroups of the step pass per item")
    pool = []
    for i in range(256):
        p = P.YgsParams.from_graph(drb1, 0, 1).path_sgd
        p.seed = 9399220 + 1000 * i
        ctx = hip.Context(drb1)
        assert ctx.setup_1d(p) == hip.OK
        pool.append(ctx)
    for n in (64, 256):
        ctxs = pool[:n]
        b = hip.Batch(ctxs)
        b.init_positions()
        b.run()
        loop = lambda: [c.sort_quality() for c in ctxs]
        batched = lambda: b.sort_quality(return_kernel_ms=True)
        assert loop() == batched()[0], "the batch's rows are not the contexts' own"      # (also the untimed call of each)
        t_loop, t_batch, k = [], [], []
        for _ in range(5):
            t_loop.append(timed_ms(loop)[0])
            t, (_, ms) = timed_ms(batched)
            t_batch.append(t)
            k.append(ms)
        print(f"    1D sorts x {n} per item: runs {' '.join('%.3f' % t for t in t_loop)} ms")
        print(f"    1D sorts x {n} batched:  runs {' '.join('%.3f' % t for t in t_batch)} ms; kernel_ms {' '.join('%.3f' % t for t in k)}")
        ml, mb = float(np.median(t_loop)), float(np.median(t_batch))
        q = b.sort_quality()[0]
        print(f"DRB1 x {n}: sort quality {ml:.3f} ms per item -> {mb:.3f} ms batched ({ml / mb:.1f}x), kernel_ms {float(np.median(k)):.3f}; "
              f"item 0: rmse {q['rmse']:.6g} bp, mae {q['mae']:.6g} bp over {q['steps']} steps", flush=True)
        b.close()
    for c in pool:
        c.close()


if __name__ == "__main__":
    main()
