"""Measures, from the oracle alone, the margin of test_gpu_layout_reference_streams.py test_full_width_quality_matches_the_oracle:
the sd of the paired difference in layout stress between two interleavings of the SAME streams (same seeds, same stream count,
so stream t draws the same terms): deterministic mode round-robin over all T streams against the two halves of the streams run
one after the other per iteration (O.State with stream_base and a quota_total split).  No GPU.  Output: profiles/r06/quality_margin.log

    python tests/measure_layout_quality_margin.py
"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from util import O, G, P, load, oracle_graph, oracle_params, gaussian_init, np_crowding
g = load("DRB1-3123.gfa"); og = oracle_graph(g)
cnt, rep, a, b = np_crowding(g); print("max cnt", cnt.max(), "a max", a.max())
T = 1216
SEEDS = [9399220 + 1000 * k for k in range(8)]
for D in (4, 8):
    p = P.LayoutSGDParams.from_graph(g, D, 1)
    print("D", D, "iter_max", p.iter_max, "mtu", p.min_term_updates, "seed", p.seed)
    c0 = gaussian_init(g, D, 7)
    s_rr, s_blk = [], []
    t0 = time.time()
    for seed in SEEDS:
        p.seed = seed
        op = oracle_params(p)
        c = c0.copy(); rc, st, _ = O.sgd_nd(og, op, c, n_streams=T); assert rc == 0
        s_rr.append(O.layout_stress(og, D, c, 100000))
        base, rem = divmod(p.min_term_updates, T)
        h = T // 2
        qa = h * base + min(rem, h); qb = p.min_term_updates - qa
        A = O.State(og, op, dims=D, n_streams=h, stream_base=0, quota_total=qa)
        B = O.State(og, op, dims=D, n_streams=T - h, stream_base=h, quota_total=qb)
        c2 = c0.copy()
        for k in range(p.iter_max + 1):
            B.run_iteration(k, c2); A.run_iteration(k, c2)
        assert A.stats().term_updates + B.stats().term_updates == st.term_updates
        assert A.stats().attempts + B.stats().attempts == st.attempts, (A.stats().attempts, B.stats().attempts, st.attempts)
        s_blk.append(O.layout_stress(og, D, c2, 100000))
    s_rr, s_blk = np.array(s_rr), np.array(s_blk)
    d = (s_blk - s_rr) / s_rr.mean()
    print("  time", time.time() - t0)
    print("  rr ", np.round(s_rr, 4), "mean", s_rr.mean(), "rel sd", s_rr.std(ddof=1) / s_rr.mean())
    print("  blk", np.round(s_blk, 4), "mean", s_blk.mean())
    print("  paired rel diff", np.round(d, 4), "mean", d.mean(), "sd", d.std(ddof=1), "4*se", 4 * d.std(ddof=1) / np.sqrt(len(SEEDS)))
