"""The layout team kernels at D = 2..8 against reference streams, in one process and from the same start.

Part 1, rates: BASELINE configs[3]'s graph (windows(1M, 64, 156250, 2)), layout parameters from the graph, `--iters` iterations
(iteration 0 first, then the range 1..iters-1 timed as bench.py's layout leg times it: one fused launch).  Per D: the team kernel at
B = 64 (GFS_F_BUNDLE(64)) and reference streams (GFS_F_BUNDLE(1)): G updates/s, kernel ms, the fraction of 8 TB/s at
40 + 32*D bytes per update, and the context's bundle / run trips / launches.
Part 2, quality (informational): at D = 4 and D = 8 on synth_bubbles(150000, 16, 9), and at D = 4 on DRB1-3123 x120, the team
kernel against reference streams at equal update counts from the same start — the ratios tests/test_gpu_layout_wide.py bounds.

--root DIR imports gfasort_amd from another tree (the parent commit's, to compare D = 2, 3 rates; where that tree has no team
kernel for a D the line says so); --label names it in the log.
    python scripts/nd_wide_probe.py [--root DIR --label TEXT] [--iters N] [--dims 2,3,...] [--no-quality] [--log FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT)
ap.add_argument("--label", default="", help="what the tree is, for the log (default: 'this tree', or 'other tree' with --root)")
ap.add_argument("--iters", type=int, default=11)
ap.add_argument("--dims", default="2,3,4,5,6,7,8")
ap.add_argument("--no-quality", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r04", "nd_wide_probe.log"))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sys.path.insert(1, ROOT)

import numpy as np   # noqa: E402
from gfasort_amd import graph as G, params as P, hip, sgd as S, quality as Q   # noqa: E402

HBM_PEAK_GBS = 8000.0
os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
log = open(args.log, "a")


def out(s):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


def timed_run(g, dims, iters, flags):
    """bench.py's layout leg: iteration 0, then 1..iters-1 in one range; returns the stats of the timed range."""
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = iters - 1
    ctx = hip.Context(g)
    try:
        ctx.setup_nd(p, hip.make_config(flags=flags))
    except hip.GfsError as e:
        ctx.close()
        return None, str(e)
    ctx.upload(S.default_layout_init(g, dims, p.seed).ravel())
    ctx.run_iteration(0)
    ctx.synchronize()
    s0 = ctx.stats()
    t0 = time.perf_counter()
    ctx.run_range(list(range(1, int(p.iter_max) + 1)))
    ctx.synchronize()
    dt = time.perf_counter() - t0
    s1 = ctx.stats()
    finite = bool(np.isfinite(ctx.download()).all())
    ctx.close()
    upd = s1.term_updates - s0.term_updates
    kms = s1.kernel_ms - s0.kernel_ms
    return dict(upd=upd, kms=kms, wall=dt, rate=upd / (kms * 1e-3) / 1e9, bundle=int(s1.bundle), run_trips=int(s1.run_trips),
                launches=int(s1.launches - s0.launches), streams=int(s1.n_streams), finite=finite,
                exact=upd == int(p.iter_max) * int(p.min_term_updates)), None


def quality(g, dims, what, iter_max=None):
    from oracle import oracle as O
    og = O.Graph(g.node_len, g.step_node, g.step_is_rev, g.path_first_step)
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    if iter_max is not None:
        p.iter_max = iter_max
    c0 = S.default_layout_init(g, dims, p.seed)
    res = {}
    for name, flags in (("ref", hip.F_BUNDLE(1)), ("team", hip.F_BUNDLE(64))):
        try:
            rc, c, st = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(flags=flags))
        except hip.GfsError as e:
            out(f"  {what} D={dims} {name}: {e}")
            return
        _, rms, _ = Q.stress_by_scale(g, c, dims, 1_000_000)
        cc = np.asarray(c).reshape(-1, 2, dims)
        err = np.abs(np.sqrt(((cc[:, 0, :] - cc[:, 1, :]) ** 2).sum(axis=1)) - g.node_len)
        res[name] = dict(stress=O.layout_stress(og, dims, c, 2_000_000), rms=rms, med=float(np.median(err)), mean=float(err.mean()),
                         rate=st.term_updates / (st.kernel_ms * 1e-3) / 1e9, upd=st.term_updates, bundle=st.bundle)
    r, t = res["ref"], res["team"]
    ratio = t["rms"] / r["rms"]
    ok = (t["stress"] <= 1.10 * r["stress"] and ratio.max() <= 1.12 and t["med"] <= 1.10 * r["med"] + 0.02 and
          t["mean"] <= 1.10 * r["mean"] + 0.02)
    out(f"  {what} D={dims} iters {p.iter_max + 1}: updates {t['upd']} / {r['upd']}  G upd/s team {t['rate']:.2f} ref {r['rate']:.2f}")
    out(f"    stress 2M pairs team/ref {t['stress']:.5f} / {r['stress']:.5f} = {t['stress'] / r['stress']:.3f} (bound 1.10)")
    out(f"    rel. error by octave team/ref: " + " ".join(f"{v:.3f}" for v in ratio) + f"  worst {ratio.max():.3f} (bound 1.12)")
    out(f"    |end-to-end - length| median {t['med']:.3f} / {r['med']:.3f}, mean {t['mean']:.3f} / {r['mean']:.3f} "
        f"(bound 1.10x + 0.02)  -> {'within the test bounds' if ok else 'OUTSIDE the test bounds'}")


label = args.label or ("this tree" if os.path.abspath(args.root) == ROOT else "other tree")
out(f"=== nd_wide_probe: {label}, {time.strftime('%Y-%m-%d %H:%M:%S')}, {hip.lib().gfs_version().decode()}")
g = G.synth_windows(1_000_000, 64, 156_250, 2)
out(f"C3 graph windows(1M,64,156250,2): {g.n_nodes} nodes, {g.n_steps} steps; {args.iters} iterations, iterations 1..{args.iters - 1} "
    f"timed in one range")
out(f"{'D':>2} {'sampler':>9} {'G upd/s':>8} {'kernel ms':>9} {'B/upd':>5} {'of 8TB/s':>8} {'bundle':>6} {'run_trips':>9} {'launches':>8} "
    f"{'streams':>7} exact finite")
rates = {}
for dims in [int(d) for d in args.dims.split(",")]:
    for name, flags in (("team B64", hip.F_BUNDLE(64)), ("ref", hip.F_BUNDLE(1))):
        r, err = timed_run(g, dims, args.iters, flags)
        if r is None:
            out(f"{dims:2d} {name:>9}  not available: {err}")
            continue
        rates[(dims, name)] = r["rate"]
        bpu = 40 + 32 * dims
        frac = r["rate"] * 1e9 * bpu / (HBM_PEAK_GBS * 1e9)
        out(f"{dims:2d} {name:>9} {r['rate']:8.2f} {r['kms']:9.2f} {bpu:5d} {frac:8.3f} {r['bundle']:6d} {r['run_trips']:9d} "
            f"{r['launches']:8d} {r['streams']:7d} {str(r['exact']):>5} {str(r['finite']):>6}")
    if (dims, "team B64") in rates and (dims, "ref") in rates:
        out(f"   D={dims}: team / reference streams = {rates[(dims, 'team B64')] / rates[(dims, 'ref')]:.2f}x")

if not args.no_quality:
    out("quality against reference streams (same start, equal update counts):")
    gb = G.synth_bubbles(150_000, 16, 9)
    for dims in (4, 8):
        quality(gb, dims, "bubbles(150000,16,9)")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import load   # noqa: E402
    quality(G.tile_series(load("DRB1-3123.gfa"), 120), 4, "DRB1-3123 x120")
log.close()
