"""Host wall time of one gfs_ctx_setup_1d, one gfs_ctx_setup_nd (D = 2) — each the first setup of a freshly created context — and
one gfs_ctx_reset_streams, on three graphs under two builds of the library, selected through GFS_LIB_PATH: one process per library,
the two alternating, two processes of each; every run and the median of 5 after gfs_warmup and one untimed round.  On the bench
headline graph also a 1D setup with a caller-supplied zeta table.

    python scripts/ctx_setup_probe.py PARENT_LIB NEW_LIB [ROUNDS] > profiles/r24/ctx_setup_probe.log 2>&1

The condition, per row and per pair of processes: the new median is not above the parent's median by more than the parent's own
spread (the slowest minus the fastest of its five).  The driver builds the graphs once and hands them to its children as .npy files
in a temporary directory; a child (--child DIR TAG) opens the GPU, the driver never does.
"""
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gfasort_amd import graph as G  # noqa: E402
from gfasort_amd import params as P  # noqa: E402

RUNS = 5
FIELDS = ("node_len", "step_node", "step_is_rev", "path_first_step")
OPS = ("setup_1d", "reset_streams", "setup_nd D=2", "setup_1d, caller's zetas")


def graphs():
    yield "DRB1-3123", G.load_gfa(os.path.join(ROOT, "tests", "data", "DRB1-3123.gfa"))
    yield "bench headline windows(1M nodes, 10M steps)", G.synth_windows(1_000_000, 64, 156_250, 2)
    yield "synth_bubbles(1500000, 32, 7): 2M nodes", G.synth_bubbles(1_500_000, 32, 7)


def child(directory, tag):
    from gfasort_amd import hip
    hip.check(hip.lib().gfs_warmup(0))
    names = open(os.path.join(directory, "names.txt")).read().splitlines()
    for k, name in enumerate(names):
        a = {f: np.load(os.path.join(directory, f"{k}_{f}.npy")) for f in FIELDS}
        g = G.FlatGraph(node_ids=np.arange(1, a["node_len"].size + 1, dtype=np.uint64), path_names=[], **a)
        sort_p, layout_p = P.YgsParams.from_graph(g, 0, 1).path_sgd, P.LayoutSGDParams.from_graph(g, 2, 1)
        zetas = hip.zeta_table(sort_p) if k == 1 else None
        ms = {op: [] for op in OPS if zetas is not None or "zetas" not in op}
        for r in range(RUNS + 1):                                   # (round 0: first use of every path, untimed)
            for op in ms:
                c = hip.Context(g)                                  # every timed setup is the first one of a fresh context
                if op == "reset_streams":
                    c.setup_1d(sort_p)
                t0 = time.perf_counter()
                if op == "setup_1d":
                    c.setup_1d(sort_p)
                elif op == "reset_streams":
                    c.reset_streams()
                elif op == "setup_nd D=2":
                    c.setup_nd(layout_p)
                else:
                    c.setup_1d(sort_p, zetas=zetas)
                dt = (time.perf_counter() - t0) * 1e3
                streams = int(c.stats().n_streams)
                c.close()
                if r:
                    ms[op].append(dt)
        for op, v in ms.items():
            print(f"RESULT\t{tag}\t{k}\t{op}\t{streams}\t" + "\t".join(f"{m:.3f}" for m in v), flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    if len(sys.argv) not in (3, 4) or sys.argv[1].startswith("-"):
        sys.exit("usage: python scripts/ctx_setup_probe.py PARENT_LIB NEW_LIB [ROUNDS]")
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    runs = {}
    with tempfile.TemporaryDirectory() as d:
        names = []
        for k, (name, g) in enumerate(graphs()):
            names.append(f"{name}: {g.n_nodes} nodes, {g.n_steps} steps, {g.n_paths} paths")
            for f in FIELDS:
                np.save(os.path.join(d, f"{k}_{f}.npy"), getattr(g, f))
        open(os.path.join(d, "names.txt"), "w").write("\n".join(names) + "\n")
        for r in range(rounds):
            for tag, lib in libs.items():
                # (a child that hangs is ended by timeout(1), which lets it go first and kills it 10 s later)
                out = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", d, tag],
                                     env=dict(os.environ, GFS_LIB_PATH=lib), stdout=subprocess.PIPE, text=True, check=True).stdout
                for line in out.splitlines():
                    if line.startswith("RESULT\t"):
                        _, t, k, op, streams, *ms = line.split("\t")
                        ms = [float(m) for m in ms]
                        runs.setdefault((int(k), op, t), []).append(ms)
                        print(f"{names[int(k)]}: {op} ({streams} streams): process {r} of {t}: " + " ".join(f"{m:9.3f}" for m in ms) +
                              f" ms | median {statistics.median(ms):.3f}", flush=True)
    failed = 0
    for (k, op, t) in sorted(runs):
        if t != "parent":
            continue
        for r, (parent, new) in enumerate(zip(runs[(k, op, "parent")], runs[(k, op, "new")])):
            mp, mn, spread = statistics.median(parent), statistics.median(new), max(parent) - min(parent)
            ok = mn <= mp + spread
            failed += not ok
            print(f"{names[k]}: {op}: pair {r}: parent median {mp:.3f} ms (spread {spread:.3f}) | new median {mn:.3f} ms "
                  f"[{min(new):.3f} .. {max(new):.3f}]: {'within' if ok else 'ABOVE'} the parent's median + spread")
    print(f"rows above the bound: {failed}")


if __name__ == "__main__":
    main()
