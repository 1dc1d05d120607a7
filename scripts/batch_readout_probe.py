"""What does the batch read-out (gfs_batch_init_positions / gfs_batch_results, K4b / K6b: batch_readout_kernels.hip) buy?

For N = 64 and 256 items of DRB1-3123 with distinct seeds at the -p Y defaults, host wall time (time.perf_counter; median of 5
after one untimed call of each) of
  * the start positions: N x Context.init_positions()                    against one Batch.init_positions()
  * the read-out:        N x (Context.download() + Context.sort_order()) against one Batch.results(), and its kernel_ms
next to the batch's SGD launch (kernel ms of one Batch.run()).  The per-item calls are the ones a batch run made before the batch
had its own.  Then, for the largest segments, one item and 64 items of 8192 nodes (a chain graph, positions of a fixed seed): the
in-LDS sort against the per-item rocPRIM path of the same call (Batch.debug_sort_cap).

usage: batch_readout_probe.py [data_dir]      default: tests/data
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip


def make(g, seed, **cfg):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.seed = seed
    ctx = hip.Context(g)
    assert ctx.setup_1d(p, hip.make_config(**cfg) if cfg else None) == hip.OK
    return ctx


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


def chain(n):
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + nid % 16)) for nid in range(n, 0, -1)]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    drb1 = G.load_gfa(os.path.join(data, "DRB1-3123.gfa"))
    print(f"DRB1-3123: {drb1.n_nodes} nodes, {drb1.n_steps} steps")
    pool = [make(drb1, 9399220 + 1000 * i) for i in range(256)]
    for n in (64, 256):
        ctxs = pool[:n]
        b = hip.Batch(ctxs)
        init_loop = median_ms(lambda: [c.init_positions() for c in ctxs], what=f"x {n} init per item")
        init_batch = median_ms(b.init_positions, what=f"x {n} init batched")
        before = b.stats()
        b.run()
        sgd_ms = b.stats().kernel_ms - before.kernel_ms
        read_loop = median_ms(lambda: [(c.download(), c.sort_order()) for c in ctxs], what=f"x {n} read-out per item")
        kernel = []
        read_batch = median_ms(lambda: kernel.append(b.results()[2]), what=f"x {n} read-out batched")
        print(f"DRB1 x {n}: init {init_loop:.3f} ms per item -> {init_batch:.3f} ms batched ({init_loop / init_batch:.1f}x) | "
              f"read-out {read_loop:.3f} ms per item -> {read_batch:.3f} ms batched ({read_loop / read_batch:.1f}x), "
              f"kernel_ms {float(np.median(kernel[1:])):.3f} | outside the SGD launch {init_loop + read_loop:.3f} -> "
              f"{init_batch + read_batch:.3f} ms, SGD launch {sgd_ms:.3f} ms", flush=True)
        b.close()
    for c in pool:
        c.close()
    g = chain(hip.SEGMENT_SORT_CAP)
    rng = np.random.default_rng(1)
    big = [make(g, i, n_streams=1) for i in range(64)]
    for c in big:
        c.upload(rng.normal(0.0, 1e4, g.n_nodes))
    for n in (1, 64):
        b = hip.Batch(big[:n])
        kernel = []
        lds = median_ms(lambda: kernel.append(b.results()[2]))
        lds_kernel = float(np.median(kernel[1:]))
        b.debug_sort_cap(64)
        kernel = []
        radix = median_ms(lambda: kernel.append(b.results()[2]))
        print(f"{hip.SEGMENT_SORT_CAP} nodes x {n}: in LDS {lds:.3f} ms (kernel_ms {lds_kernel:.3f}) | per-item rocPRIM in the same call "
              f"{radix:.3f} ms (events {float(np.median(kernel[1:])):.3f})", flush=True)
        b.close()


if __name__ == "__main__":
    main()
