"""What does the batched diagnosis (gfs_batch_path_errors / gfs_batch_stretched_pairs / gfs_batch_node_errors, K7h / K7i / K7j:
batch_diagnosis_kernels.hip) buy?

For N = 64 and 256 items of DRB1-3123 with distinct seeds, set up as 1D sorts and as 2-D layouts at the policy's width and run
once as a batch, host wall time (time.perf_counter; median of 5 after one untimed call of each) at z = 1, ratio 10 of
  * per path:   N x Context.path_errors()              against one Batch.path_errors(), and its kernel_ms
  * the pairs:  N x Context.stretched_pairs(cap = 20)  against one Batch.stretched_pairs(cap = 20), and its kernel_ms
  * per node:   N x Context.node_errors()              against one Batch.node_errors(), and its kernel_ms
The per-item calls are the only way a batch had before it had its own.

With a second argument, the path of a gfasort_hip binary: `gfasort_hip --batch LIST -p Y --iter-max 2 --diagnose -v 0` over 64 copies
of DRB1-3123 end to end, five runs, wall time of each (run it once per binary to compare two builds).

usage: batch_diagnosis_probe.py [data_dir [gfasort_hip]]      default: tests/data
"""
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip


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


def cli_runs(cli, gfa, n=64, runs=5):
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "list.tsv")
        with open(lst, "w") as fh:
            for i in range(n):
                fh.write(f"{gfa}\t{tmp}/out_{i}.gfa\n")
        times = []
        for _ in range(runs):
            t0 = time.perf_counter()
            r = subprocess.run([cli, "--batch", lst, "-p", "Y", "--iter-max", "2", "--diagnose", "-v", "0"], capture_output=True, text=True)
            times.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-2000:]
        print(f"{cli} --batch --diagnose over {n} x DRB1: runs {' '.join('%.3f' % t for t in times)} s, median {float(np.median(times)):.3f} s",
              flush=True)


def main():
    data = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "data")
    drb1 = G.load_gfa(os.path.join(data, "DRB1-3123.gfa"))
    print(f"DRB1-3123: {drb1.n_nodes} nodes, {drb1.n_steps} steps, {drb1.n_paths} paths, {-(-drb1.n_steps // 512)} tiles; z = 1, ratio 10")
    for dims in (0, 2):
        pool = []
        for i in range(256):
            p = P.LayoutSGDParams.from_graph(drb1, 2, 1) if dims else P.YgsParams.from_graph(drb1, 0, 1).path_sgd
            p.seed = 9399220 + 1000 * i
            p.iter_max = 2
            ctx = hip.Context(drb1)
            assert (ctx.setup_nd if dims else ctx.setup_1d)(p) == hip.OK
            if dims == 0:
                ctx.init_positions()
            pool.append(ctx)
        kind = "2-D layouts" if dims else "1D sorts"
        for n in (64, 256):
            ctxs = pool[:n]
            b = hip.Batch(ctxs)
            b.run()
            row = []
            for name, loop, batched in (
                    ("paths", lambda: [c.path_errors(1, 10.0) for c in ctxs], lambda: b.path_errors(1, 10.0, return_ms=True)[-1]),
                    ("pairs", lambda: [c.stretched_pairs(1, 10.0, cap=20) for c in ctxs], lambda: b.stretched_pairs(1, 10.0, cap=20, return_ms=True)[-1]),
                    ("nodes", lambda: [c.node_errors(1, 10.0) for c in ctxs], lambda: b.node_errors(1, 10.0, return_ms=True)[-1])):
                t_loop = median_ms(loop, what=f"{kind} x {n} {name} per item")
                k = []
                t_batch = median_ms(lambda: k.append(batched()), what=f"{kind} x {n} {name} batched")
                row.append(f"{name} {t_loop:.3f} ms per item -> {t_batch:.3f} ms batched ({t_loop / t_batch:.1f}x), kernel_ms {float(np.median(k[1:])):.3f}")
            print(f"DRB1 x {n}, {kind}: " + " | ".join(row), flush=True)
            b.close()
        for c in pool:
            c.close()
    if len(sys.argv) > 2:
        cli_runs(sys.argv[2], os.path.join(data, "DRB1-3123.gfa"))


if __name__ == "__main__":
    main()
