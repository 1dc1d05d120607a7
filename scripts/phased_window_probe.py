"""Choosing GFS_F_PHASED's default window (host_tables.hip gfs_phase_window): candidate windows around the reference's switch to the
cooling phase, f = first_cooling = floor(cooling_start * iter_max), run through the fused phased kernel (K1e), against reference
streams (GFS_F_BUNDLE(1)) of the same seed.  Printed per run: kernel ms and the figures of tests/test_gpu_quality.py _compare
(sampled stress 2M pairs, worst ratio of the relative error per octave of path distance and the ratio at distance 1, RMSE / MAE of
the sort, Kendall tau, Spearman rho) — nothing is asserted.

    python scripts/phased_window_probe.py [--seeds N] [--graphs drb1,drb1s,bubbles] [--iter-max 100]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from util import O, G, P, load, oracle_graph  # noqa: E402
from gfasort_amd import hip, quality as Q  # noqa: E402


def figures(g, og, x_ref, x_new):
    s_ref, s_new = O.stress_1d(og, x_ref, 2_000_000), O.stress_1d(og, x_new, 2_000_000)
    pr = Q.stress_by_scale(g, x_ref, 0, 1_000_000)[1]
    pn = Q.stress_by_scale(g, x_new, 0, 1_000_000)[1]
    o_ref, o_new = hip.sort_order(x_ref).astype(np.int64), hip.sort_order(x_new).astype(np.int64)
    q_ref, q_new = Q.layout_quality(g, o_ref), Q.layout_quality(g, o_new)
    r_ref = Q.ranks_of(o_ref)
    r_new = Q.oriented(r_ref, Q.ranks_of(o_new))
    return dict(stress=s_new / s_ref, d1=float(pn[0] / pr[0]), worst=float(np.max(pn / pr)), rmse=q_new["rmse"] / q_ref["rmse"],
                mae=q_new["mae"] / q_ref["mae"], tau=Q.kendall_tau(r_ref, r_new), rho=Q.spearman_rho(r_ref, r_new),
                rmse_bp=q_new["rmse"])


def run(ctx, p, flags, window=None):
    ctx.setup_1d(p, hip.make_config(flags=flags))
    if window is not None:
        ctx.phase_window(*window)
    ctx.init_positions()
    ctx.run()
    return ctx.download(), ctx.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--graphs", default="drb1,drb1s,bubbles")
    ap.add_argument("--iter-max", type=int, default=100)
    args = ap.parse_args()
    graphs = {"drb1": lambda: G.tile_series(load("DRB1-3123.gfa"), 120),
              "drb1s": lambda: G.tile_series(load("DRB1-3123.gfa"), 120, shuffle_seed=17),
              "bubbles": lambda: G.synth_bubbles(400_000, 24, 6)}
    for name in args.graphs.split(","):
        g = graphs[name]()
        og = oracle_graph(g)
        ctx = hip.Context(g)
        p0 = P.YgsParams.from_graph(g, 0, 1).path_sgd
        p0.iter_max = args.iter_max
        n = p0.iter_max
        f = int(np.floor(p0.cooling_start * n))
        wins = [("f-10%,f+20%", f - n // 10, f + n // 5), ("f-10%,f+10%", f - n // 10, f + n // 10), ("f,f+20%", f, f + n // 5),
                ("f+1,f+1+30%", f + 1, f + 1 + 3 * n // 10), ("f+1,end", f + 1, n + 1), ("empty (team)", 0, 0)]
        print(f"== {name}: {g.n_nodes} nodes, iter_max {n}, first_cooling {f}", flush=True)
        for s in range(args.seeds):
            p = P.YgsParams.from_graph(g, 0, 1).path_sgd
            p.iter_max = args.iter_max
            p.seed = p0.seed + s
            run(ctx, p, hip.F_BUNDLE(1))                            # warm-up
            x_ref, st_ref = run(ctx, p, hip.F_BUNDLE(1))
            ms_ref = st_ref.kernel_ms
            print(f"  seed {p.seed}: reference streams {st_ref.n_streams} streams, kernel {ms_ref:.1f} ms", flush=True)
            for label, b, e in wins:
                b, e = max(0, b), min(n + 1, e)
                t0 = time.time()
                x, st = run(ctx, p, hip.F_PHASED, (b, e))
                assert st.term_updates == (n + 1) * p.min_term_updates and st.launches >= 1
                fg = figures(g, og, x_ref, x)
                print(f"    [{b:3d},{e:3d}) {label:13s} kernel {st.kernel_ms:6.1f} ms ({st.kernel_ms / ms_ref:.2f} x ref)  stress x{fg['stress']:.3f}"
                      f"  d=1 x{fg['d1']:.3f}  worst octave x{fg['worst']:.3f}  rmse x{fg['rmse']:.3f} ({fg['rmse_bp']:.0f} bp)"
                      f"  mae x{fg['mae']:.3f}  tau {fg['tau']:.4f} rho {fg['rho']:.4f}  ({time.time() - t0:.0f} s)", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
