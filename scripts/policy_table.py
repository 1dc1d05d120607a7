#!/usr/bin/env python3
"""What the launch policy decides, cell by cell, through the public Python API only: runs unchanged at two commits, the two
outputs are compared line for line.  Run from the root of the tree to be measured: python scripts/policy_table.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from gfasort_amd import graph as G, hip, params as P   # noqa: E402


def synth(n_nodes, mix):
    """mix: [(how many paths, steps each)]; path p walks consecutive nodes from a start spread over the graph."""
    counts = np.array([c for n, c in mix for _ in range(n)], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    starts = (np.arange(len(counts), dtype=np.int64) * 2654435761) % n_nodes
    step_node = np.concatenate([(s + np.arange(c)) % n_nodes for s, c in zip(starts, counts)]).astype(np.uint32)
    node_len = (1 + np.arange(n_nodes) % 5).astype(np.uint32)
    return G.FlatGraph(node_len=node_len, step_node=step_node, step_is_rev=np.zeros(len(step_node), dtype=np.uint8),
                       path_first_step=first, node_ids=np.arange(1, n_nodes + 1, dtype=np.uint64))


MIXES = {"B64": [(16, 4096)], "B32": [(512, 128)], "B16": [(1024, 64)], "B8": [(2048, 32)], "B4": [(4096, 16)], "B1": [(8192, 8)],
         "B32mixed": [(15, 4096), (32, 128)]}
FLAGS = {"default": {}, "bundle8": {"flags": hip.F_BUNDLE(8)}, "bundle64": {"flags": hip.F_BUNDLE(64)}, "phased": {"flags": hip.F_PHASED},
         "no_fuse": {"flags": hip.F_NO_FUSE}, "free_running": {"flags": hip.F_DBG_FREE_RUNNING}, "plain_loads": {"flags": hip.F_PLAIN_LOADS},
         "no_lds": {"flags": hip.F_NO_LDS_TABLES}, "trace": {"trace_per_stream": 2}, "streams_above_residency": {"n_streams": 327680},
         "phased_free_running": {"flags": hip.F_PHASED | hip.F_DBG_FREE_RUNNING}}


def params(g, dims, quota):
    mx = int(g.path_step_counts().max())
    kw = dict(iter_max=3, min_term_updates=quota, eta_max=float(mx * mx), space=mx, space_max=100, space_quantization_step=100, seed=4242)
    return P.LayoutSGDParams(dimensions=dims, **kw) if dims else P.PathSGDParams(**kw)


def run(g, dims, quota, cfg_kw, want_hash):
    p = params(g, dims, quota)
    ctx = hip.Context(g)
    try:
        cfg = hip.make_config(**cfg_kw)
        rc = ctx.setup_nd(p, cfg) if dims else ctx.setup_1d(p, cfg)
        if rc == hip.NOTHING_TO_DO:
            return "nothing to do"
        if dims:
            ctx.upload(hip.init_layout(g, dims, 7))
        else:
            ctx.init_positions()
        window = "-"
        if cfg_kw.get("flags", 0) & hip.F_PHASED:
            window = "[%d,%d)" % ctx.phase_window()
        ctx.run()
        st = ctx.stats()
        out = (f"n_streams={st.n_streams} bundle={st.bundle} run_trips={st.run_trips} window={window} launches={st.launches} "
               f"iterations={st.iterations} term_updates={st.term_updates}")
        if want_hash:
            out += " sha256=" + hashlib.sha256(ctx.download().tobytes()).hexdigest()[:32]
        return out
    except hip.GfsError as e:
        return "error: " + str(e)
    finally:
        ctx.close()


def main():
    cells = []
    for n_nodes in (16320, 16384, 66000):
        for mix in MIXES:
            for dims in (0, 2, 3, 5):
                cells.append((n_nodes, mix, dims, "default"))
    for n_nodes in (16384, 66000):
        for mix in ("B64", "B1"):
            for dims in (0, 2, 5):
                for name in FLAGS:
                    if name != "default":
                        cells.append((n_nodes, mix, dims, name))
    graphs = {}
    for n_nodes, mix, dims, name in cells:
        if (n_nodes, mix) not in graphs:
            graphs[(n_nodes, mix)] = synth(n_nodes, MIXES[mix])
        g = graphs[(n_nodes, mix)]
        for quota in ((4096, 2000000) if "n_streams" not in FLAGS[name] else (2000000,)):
            label = f"nodes={n_nodes} mix={mix} dims={dims} flags={name} quota={quota}"
            print(label, "|", run(g, dims, quota, dict(FLAGS[name]), False), flush=True)
        if "n_streams" not in FLAGS[name]:
            one_wave = dict(FLAGS[name], n_streams=64)                    # a single wave is deterministic: its positions, hashed
            print(f"nodes={n_nodes} mix={mix} dims={dims} flags={name} quota=4096 one wave", "|", run(g, dims, 4096, one_wave, True), flush=True)


if __name__ == "__main__":
    main()
