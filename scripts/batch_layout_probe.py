"""What do the batch's packed coordinates (gfs_batch_upload_coords / gfs_batch_coords, K4c / K6c) and its batched pair errors
(gfs_batch_pair_errors, K7g: batch_quality_kernels.hip) buy?

For N = 64 and 256 items of DRB1-3123 with distinct seeds, set up as 2-D layouts at the policy's width, host wall time
(time.perf_counter; median of 5 after one untimed call of each) of
  * the start coordinates: N x Context.upload()       against one Batch.upload_coords()
  * the read-out:          N x Context.download()     against one Batch.coords(), and its kernel_ms
  * the quality:           N x Context.pair_errors()  against one Batch.pair_errors(), at the default step-distance ladder,
                           and its kernel_ms
next to the batch's SGD launch (kernel ms of one Batch.run()).  The per-item calls are the ones a batch of layouts made before
the batch had its own.

usage: batch_layout_probe.py [data_dir]      default: tests/data
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip, quality as Q, sgd as S


def median_ms(f, runs=5, what=None):
    f()                                                        # untimed: code objects, scratch
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    if what:
        print(f"    {what}: runs {' '.join('%.3f' % t for t in times)} ms", flush=True)
    return float(np.median(times))


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    drb1 = G.load_gfa(os.path.join(data, "DRB1-3123.gfa"))
    zs = Q.step_distance_ladder(int(np.diff(drb1.path_first_step.astype(np.int64)).max()))
    print(f"DRB1-3123: {drb1.n_nodes} nodes, {drb1.n_steps} steps, D = 2, {len(zs)} step distances")
    pool, starts = [], []
    for i in range(256):
        p = P.LayoutSGDParams.from_graph(drb1, 2, 1)
        p.seed = 9399220 + 1000 * i
        ctx = hip.Context(drb1)
        assert ctx.setup_nd(p) == hip.OK
        pool.append(ctx)
        starts.append(S.default_layout_init(drb1, 2, p.seed) if i < 8 else starts[i % 8])
    for n in (64, 256):
        ctxs, c0 = pool[:n], starts[:n]
        b = hip.Batch(ctxs)
        up_loop = median_ms(lambda: [c.upload(x) for c, x in zip(ctxs, c0)], what=f"x {n} upload per item")
        up_batch = median_ms(lambda: b.upload_coords(c0), what=f"x {n} upload batched")
        before = b.stats()
        b.run()
        sgd_ms = b.stats().kernel_ms - before.kernel_ms
        down_loop = median_ms(lambda: [c.download() for c in ctxs], what=f"x {n} read-out per item")
        k_down = []
        down_batch = median_ms(lambda: k_down.append(b.coords()[1]), what=f"x {n} read-out batched")
        q_loop = median_ms(lambda: [c.pair_errors(zs) for c in ctxs], what=f"x {n} pair errors per item")
        k_q = []
        q_batch = median_ms(lambda: k_q.append(b.pair_errors(zs, return_ms=True)[1]), what=f"x {n} pair errors batched")
        print(f"DRB1 x {n}: upload {up_loop:.3f} ms per item -> {up_batch:.3f} ms batched ({up_loop / up_batch:.1f}x) | "
              f"read-out {down_loop:.3f} -> {down_batch:.3f} ms ({down_loop / down_batch:.1f}x), kernel_ms {float(np.median(k_down[1:])):.3f} | "
              f"pair errors {q_loop:.3f} -> {q_batch:.3f} ms ({q_loop / q_batch:.1f}x), kernel_ms {float(np.median(k_q[1:])):.3f} | "
              f"all three {up_loop + down_loop + q_loop:.3f} -> {up_batch + down_batch + q_batch:.3f} ms, SGD launch {sgd_ms:.3f} ms", flush=True)
        b.close()
    for c in pool:
        c.close()


if __name__ == "__main__":
    main()
