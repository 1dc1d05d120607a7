"""Host wall time of gfs_ctx_create (hip.Context(g)) on three graphs under two builds of the library, selected through GFS_LIB_PATH:
one process per library, the two alternating, every run and the median of 5 after gfs_warmup.  GFS_TIMING laps of one more create
of each graph go to stderr, which the log keeps.

    python scripts/ctx_create_probe.py PARENT_LIB NEW_LIB [ROUNDS] > profiles/r21/ctx_create_probe.log 2>&1

The driver builds the graphs once and hands them to its children as .npy files in a temporary directory; a child (--child DIR TAG)
opens the GPU, the driver never does.
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

RUNS = 5
FIELDS = ("node_len", "step_node", "step_is_rev", "path_first_step")


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
        hip.Context(g).close()                                  # (first use of the path)
        ms = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            c = hip.Context(g)
            ms.append((time.perf_counter() - t0) * 1e3)
            c.close()
        print(f"RESULT\t{tag}\t{k}\t" + "\t".join(f"{m:.3f}" for m in ms), flush=True)
        os.environ["GFS_TIMING"] = "1"                          # the laps of one more create, after the timed ones
        sys.stderr.write(f"[laps] {tag}: {name}\n")
        sys.stderr.flush()
        hip.Context(g).close()
        del os.environ["GFS_TIMING"]


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    if len(sys.argv) not in (3, 4) or sys.argv[1].startswith("-"):
        sys.exit("usage: python scripts/ctx_create_probe.py PARENT_LIB NEW_LIB [ROUNDS]")
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
                        _, t, k, *ms = line.split("\t")
                        ms = [float(m) for m in ms]
                        runs.setdefault((int(k), t), []).append(ms)
                        print(f"{names[int(k)]}: process {r} of {t}: " + " ".join(f"{m:9.3f}" for m in ms) + f" ms | median {statistics.median(ms):.3f}")
    for k, name in enumerate(names):
        parent, new = runs[(k, "parent")], runs[(k, "new")]
        slowest = max(max(ms) for ms in parent)
        meds_p, meds_n = [statistics.median(ms) for ms in parent], [statistics.median(ms) for ms in new]
        verdict = "within" if max(meds_n) <= slowest else "ABOVE"
        print(f"{name}: parent medians {meds_p} (slowest run {slowest:.3f}) | new medians {meds_n}: {verdict} the parent's slowest run")


if __name__ == "__main__":
    main()
