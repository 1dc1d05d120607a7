"""What does the device quality read-out (K7, quality_kernels.hip) cost?  On the bench graph, after the default sort and after the
default 2-D layout: the default ladder and a single z = 1 pass, kernels timed by HIP events (GFS_TIMING's line of
gfs_ctx_pair_errors), the first call and a repeat; the repeat as a fraction of 8 TB/s at 32 B of records + 16 * max(D, 1) B of
positions per pair; beside them the wall time of the host's quality.step_distance_errors at z = 1 on the same positions.

usage: readout_probe.py [n_nodes n_paths window seed]      default: 1000000 64 156250 2 (bench.py's graph)
"""
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gfasort_amd import graph as G, params as P, hip, quality as Q

PEAK = 8e12


def kernels_ms(fn):
    """Runs fn() with GFS_TIMING set and returns (its result, the kernels' milliseconds the library printed on stderr)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GFS_TIMING"] = "1"
        try:
            out = fn()
        finally:
            del os.environ["GFS_TIMING"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode()
    return out, sum(float(v) for v in re.findall(r"\[gfs_ctx_pair_errors\].*kernels (\S+) ms", text))


def measure(ctx, dims, label):
    g = ctx.graph
    per_pair = 32 + 16 * max(dims, 1)
    ladder = Q.step_distance_ladder(int(np.diff(g.path_first_step.astype(np.int64)).max()))
    for name, zs in (("z = 1", [1]), (f"ladder of {len(ladder)}", ladder)):
        rows, first = kernels_ms(lambda: ctx.pair_errors(zs))
        reps = [kernels_ms(lambda: ctx.pair_errors(zs))[1] for _ in range(5)]
        rep = sorted(reps)[len(reps) // 2]
        pairs = int(rows["pairs"].sum())
        print(f"{label} {name}: {pairs} pairs; kernels first call {first:.4f} ms, repeat {rep:.4f} ms (median of 5: "
              f"{' '.join('%.4f' % v for v in reps)}); {pairs * per_pair / (rep * 1e-3) / 1e12:.3f} TB/s at {per_pair} B per pair = "
              f"{pairs * per_pair / (rep * 1e-3) / PEAK:.3f} of 8 TB/s")
    t0 = time.perf_counter()
    rows = ctx.pair_errors([1])
    print(f"{label} z = 1 wall time of the call (scratch resident): {(time.perf_counter() - t0) * 1e3:.3f} ms")
    x = ctx.download()
    t0 = time.perf_counter()
    e2 = Q.step_distance_errors(g, x, dims, 1)
    host = time.perf_counter() - t0
    print(f"{label} z = 1 on the host (quality.step_distance_errors, numpy): {host * 1e3:.1f} ms; rms {np.sqrt(e2.mean()):.6g} "
          f"device rms {np.sqrt(rows['sum_rel_sq'][0] / rows['pairs'][0]):.6g} pairs {e2.size} / {int(rows['pairs'][0])}")
    for r in Q.device_profile(ctx)[:6]:
        print("   ", r)


def main():
    a = [int(v) for v in sys.argv[1:5]] if len(sys.argv) >= 5 else [1_000_000, 64, 156_250, 2]
    g = G.synth_windows(*a)
    print(f"graph synth_windows{tuple(a)}: {g.n_nodes} nodes, {g.n_steps} steps, {g.n_paths} paths")
    ctx = hip.Context(g)
    ctx.setup_1d(P.YgsParams.from_graph(g, 0, 1).path_sgd)
    ctx.init_positions()
    ctx.run()
    print(f"sort: kernels {ctx.stats().kernel_ms:.2f} ms")
    measure(ctx, 0, "1D sort")
    t0 = time.perf_counter()
    q = ctx.sort_quality()
    print(f"1D sort_quality wall {(time.perf_counter() - t0) * 1e3:.2f} ms: rmse {q['rmse']:.6g} mae {q['mae']:.6g} steps {q['steps']}")
    t0 = time.perf_counter()
    s = ctx.sampled_stress()
    print(f"1D sampled_stress (10000 samples) wall {(time.perf_counter() - t0) * 1e3:.2f} ms: {s:.6f}")
    pl = P.LayoutSGDParams.from_graph(g, 2, 1)
    ctx.setup_nd(pl)
    ctx.upload(hip.init_layout(g, 2, pl.seed))
    ctx.run()
    print(f"2-D layout: kernels {ctx.stats().kernel_ms:.2f} ms")
    measure(ctx, 2, "2-D layout")
    ctx.close()


if __name__ == "__main__":
    main()
