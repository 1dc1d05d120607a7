"""Shared helpers for the parity tests: oracle <-> product parameter plumbing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402  (tests are allowed to use the oracle)
from gfasort_amd import graph as G  # noqa: E402
from gfasort_amd import params as P  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_FIELDS = ["iter_max", "iter_with_max_learning_rate", "min_term_updates", "delta", "eps", "eta_max", "theta",
           "space", "space_max", "space_quantization_step", "cooling_start", "nthreads", "seed"]


def oracle_params(p, dimensions=2):
    kw = {k: getattr(p, k) for k in _FIELDS}
    kw["dimensions"] = getattr(p, "dimensions", dimensions)
    return O.params(**kw)


def oracle_graph(g):
    return O.Graph(g.node_len, g.step_node, g.step_is_rev, g.path_first_step)


def load(name):
    return G.load_gfa(os.path.join(DATA, name))


def cli_solo_and_batch(cli, tmp_path, names, flags, layouts):
    """One `-i/-o` run per fixture (solo_NAME, and solo_NAME.tsv for a layout), then one `--batch LIST` run over all of them
    (batch_NAME, batch_NAME.tsv), with the same flags.  Returns the completed processes: the solo ones, the batch's."""
    import subprocess
    solo, lines = [], []
    for name in names:
        src = os.path.join(DATA, name)
        cmd = [cli, "-i", src, "-o", str(tmp_path / ("solo_" + name))] + flags
        if layouts:
            cmd += ["--layout-out", str(tmp_path / ("solo_" + name + ".tsv"))]
        solo.append(subprocess.run(cmd, capture_output=True, text=True))
        lines.append("\t".join([src, str(tmp_path / ("batch_" + name))] + ([str(tmp_path / ("batch_" + name + ".tsv"))] if layouts else [])) + "\n")
    (tmp_path / "list.tsv").write_text("".join(lines))
    return solo, subprocess.run([cli, "--batch", str(tmp_path / "list.tsv")] + flags, capture_output=True, text=True)


def gaussian_init(g, dims, seed):
    """Caller-side init of layout dims >= 1 (the reference uses rand_distr StandardNormal, which is
    not restated): Box-Muller on SplitMix64(seed), scaled by sqrt(2N) like sgd.rs:836."""
    n = g.n_nodes * 2 * dims
    r = G.splitmix64_array(seed, 2 * n)
    u1 = ((r[:n] >> np.uint64(11)).astype(np.float64) + 1.0) / 9007199254740993.0
    u2 = (r[n:] >> np.uint64(11)).astype(np.float64) / 9007199254740992.0
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    c = (z * np.sqrt(2.0 * g.n_nodes)).reshape(g.n_nodes, 2, dims)
    og = oracle_graph(g)
    c0 = O.init_layout_dim0(og, dims).reshape(g.n_nodes, 2, dims)
    c[:, :, 0] = c0[:, :, 0]
    return np.ascontiguousarray(c.reshape(-1))


# ---- graphs and a restatement for the crowding exponents and the 55-bit step positions (sgd_device.h crowd_shift) ----
NO_NODE = 0xFFFFFFFF


def graph_from_paths(paths, node_len, rev=None):
    """FlatGraph from explicit paths (lists of dense node indices or NO_NODE)."""
    steps = [n for pth in paths for n in pth]
    first = np.concatenate([[0], np.cumsum([len(pth) for pth in paths])]).astype(np.uint64)
    node_len = np.asarray(node_len, dtype=np.uint32)
    is_rev = np.zeros(len(steps), dtype=np.uint8) if rev is None else np.asarray(rev, dtype=np.uint8)
    return G.FlatGraph(node_len=node_len, step_node=np.asarray(steps, dtype=np.uint32), step_is_rev=is_rev,
                       path_first_step=first, node_ids=np.arange(1, len(node_len) + 1, dtype=np.uint64),
                       path_names=[f"p{i}" for i in range(len(paths))])


def crowding_edge_graph(seed=5):
    """One edge case of the crowding statistics per path.  Returns (graph, expected) with expected[name] = (node, cnt, rep)
    for the named nodes.  Fillers are fresh nodes, visited once."""
    rng = np.random.default_rng(seed)
    nxt = [0]

    def fresh(k=1):
        out = list(range(nxt[0], nxt[0] + k))
        nxt[0] += k
        return out
    named, paths = {}, []

    def node(name):
        named[name] = fresh()[0]
        return named[name]
    a63, a64 = node("dist63"), node("dist64")
    paths.append(fresh(3) + [a63] + fresh(62) + [a63] + fresh(5) + [a64] + fresh(63) + [a64] + fresh(3))
    paths.append([])                                                   # empty paths between non-empty ones
    edge = node("path_edge")                                           # ends one path, starts the next
    paths.append(fresh(10) + [edge])
    paths.append([])
    paths.append([edge] + fresh(10))
    hole = node("no_node_window")                                      # NO_NODE steps inside a repeat window
    paths.append(fresh(2) + [hole] + [NO_NODE] * 20 + [hole] + [NO_NODE] * 41 + [hole] + [NO_NODE] * 5 + fresh(2))
    paths.append([NO_NODE] * 3)                                        # a path of absent nodes only
    for name, c in (("cnt16", 16), ("cnt17", 17), ("cnt32", 32), ("cnt33", 33)):   # cnt 2^k and 2^k + 1, rep 1
        n = node(name)
        pth = []
        for _ in range(c):
            pth += [n] + fresh(64)
        paths.append(pth)
    for name, c in (("rep2", 2), ("rep4", 4), ("rep5", 5), ("rep8", 8), ("rep9", 9), ("rep64", 64)):   # rep 2^k, 2^k + 1
        n = node(name)
        gap = max(1, 64 // c - 1) if c < 64 else 0
        pth = fresh(2)
        for _ in range(c):
            pth += [n] + fresh(gap)
        paths.append(pth[:2] + pth[2:] + fresh(70))
    hub = node("hub")                                                  # cnt > 2^16, spread over many paths
    filler = fresh(3)
    for _ in range(40):
        pth = []
        for _ in range(1700):
            pth += [hub] + filler
        paths.append(pth)
    node_len = rng.integers(1, 17, nxt[0]).astype(np.uint32)
    g = graph_from_paths(paths, node_len, rev=None)
    g.step_is_rev = (rng.random(g.n_steps) < 0.3).astype(np.uint8)
    expected = {"dist63": (2, 2), "dist64": (2, 1), "path_edge": (2, 1), "no_node_window": (3, 3),
                "cnt16": (16, 1), "cnt17": (17, 1), "cnt32": (32, 1), "cnt33": (33, 1),
                "rep2": (2, 2), "rep4": (4, 4), "rep5": (5, 5), "rep8": (8, 8), "rep9": (9, 9), "rep64": (64, 64),
                "hub": (68000, 16)}
    return g, {k: (named[k],) + v for k, v in expected.items()}


def hub_graph(n=3000, n_paths=6, every=4, seed=3):
    """A chain of n nodes that n_paths paths traverse, each stepping on one hub node after every `every`-th step."""
    rng = np.random.default_rng(seed)
    hub = n
    paths = []
    for _ in range(n_paths):
        pth = []
        for k in range(n):
            pth.append(k)
            if k % every == every - 1:
                pth.append(hub)
        paths.append(pth)
    return graph_from_paths(paths, rng.integers(1, 17, n + 1))


def np_crowding(g):
    """Per dense node: cnt (steps on it), rep (most visits within the 63 steps before a step and the step itself, inside its
    path), and the exponents a = ceil(log2 cnt) <= 63, b = ceil(log2 rep) <= 7 (0 for cnt, rep <= 1)."""
    sn = g.step_node.astype(np.int64)
    S = sn.shape[0]
    present = sn != NO_NODE
    cnt = np.bincount(sn[present], minlength=g.n_nodes)
    first = g.path_first_step.astype(np.int64)
    path_start = np.repeat(first[:-1], np.diff(first)) if S else np.zeros(0, np.int64)
    c = np.ones(S, dtype=np.int64)
    idx = np.arange(S)
    for d in range(1, 64):
        ok = idx - d >= path_start
        same = np.zeros(S, dtype=bool)
        same[d:] = sn[d:] == sn[:-d]
        c += ok & same & present
    rep = np.zeros(g.n_nodes, dtype=np.int64)
    np.maximum.at(rep, sn[present], c[present])

    def clog2(v, hi):
        v = np.asarray(v, dtype=np.float64)
        out = np.where(v <= 1, 0, np.ceil(np.log2(np.maximum(v, 1))))
        return np.minimum(out, hi).astype(np.int64)
    return cnt, rep, clog2(cnt, 63), clog2(rep, 7)


# ---- the layout update, restated without the oracle (tests/test_layout_update_restatement.py) ----
def replay_layout_trace(c0, D, trace, etas, updates_per_iteration):
    """One stream's layout updates replayed from its trace of terms (i, j, d_ij): the arithmetic of sgd.rs:1085-1149 as read
    from the reference, in Python floats (IEEE doubles, one rounding per operation, no fused multiply-add) and math.sqrt
    (correctly rounded) only.  c0: Layout order, c[(2 * node + end) * D + k]; i and j are the reference's 2 * node + end
    (sgd.rs:1099-1103).  The n-th term runs at etas[n // updates_per_iteration].  No crowding term: the reference has none.
    Returns the final coordinates as a new float64 array."""
    import math
    c = [float(v) for v in np.asarray(c0, dtype=np.float64)]
    ti = [int(v) for v in trace["i"]]
    tj = [int(v) for v in trace["j"]]
    td = [float(v) for v in trace["d_ij"]]
    etas = [float(v) for v in etas]
    dims = range(D)
    for n in range(len(ti)):
        eta = etas[n // updates_per_iteration]
        d_ij = td[n]
        term_weight = 1.0 / d_ij                               # sgd.rs:1085
        mu = min(eta * term_weight, 1.0)                       # :1086
        bi, bj = ti[n] * D, tj[n] * D                          # :1102-1103, coords[d][idx]
        deltas = [0.0] * D                                     # :1106
        mag_sq = 0.0                                           # :1107
        for k in dims:                                         # :1108-1113
            deltas[k] = c[bi + k] - c[bj + k]
            mag_sq += deltas[k] * deltas[k]
        if mag_sq == 0.0:                                      # :1116-1119
            deltas[0] = 1e-9
            mag_sq = 1e-18
        mag = math.sqrt(mag_sq)                                # :1121
        delta_update = mu * (mag - d_ij) / 2.0                 # :1125
        r = delta_update / mag                                 # :1142
        for k in dims:                                         # :1143-1149
            r_d = r * deltas[k]
            c_i = c[bi + k]                                    # both ends are read before either is written,
            c_j = c[bj + k]
            c[bi + k] = c_i - r_d
            c[bj + k] = c_j + r_d                              # so the second store wins where i == j
    return np.array(c, dtype=np.float64)


def self_loop_graph():
    """One path that steps on nodes twice, also twice in a row: layout terms with i == j occur (sgd.rs:1143-1149)."""
    txt = "".join(f"S\t{i}\t{'ACGT'[:1 + i % 4]}\n" for i in range(1, 9)) + \
        "P\tp\t1+,2+,3+,2+,3-,4+,4+,5+,1-,6+,7+,8+,7-,8+\t*\n"
    return G.parse_gfa(txt)


def absent_node_graph():
    """A path with one step on an id that is no node (skipped, sgd.rs:525-538; costs no bp, sgd.rs:52-54) and a one-step path."""
    txt = "".join(f"S\t{i}\t{'A' * (1 + i % 5)}\n" for i in range(1, 41)) + \
        "P\tp\t" + ",".join(f"{i}+" for i in list(range(1, 21)) + [99] + list(range(21, 41))) + "\t*\n" + \
        "P\tq\t7+\t*\n"
    return G.parse_gfa(txt)


def reverse_short_paths_graph():
    """One long path and 4000 paths of 12 steps over 6000 nodes, 30 % of the steps reverse (the graph of
    test_gpu_parity.py test_reverse_steps_and_short_paths_mix)."""
    rng = np.random.default_rng(5)
    n = 6000
    lens = rng.integers(1, 9, n).astype(np.uint32)
    long_path = np.arange(n, dtype=np.uint32)
    shorts = [np.arange(s, s + 12, dtype=np.uint32) for s in rng.integers(0, n - 12, 4000)]
    steps = np.concatenate([long_path] + shorts)
    firsts = np.concatenate([[0], np.cumsum([len(long_path)] + [12] * len(shorts))]).astype(np.uint64)
    rev = (rng.random(steps.shape[0]) < 0.3).astype(np.uint8)
    return G.FlatGraph(node_len=lens, step_node=steps, step_is_rev=rev, path_first_step=firsts,
                       node_ids=np.arange(1, n + 1, dtype=np.uint64), path_names=[f"p{k}" for k in range(len(shorts) + 1)])


def single_stream_kshift(g):
    """The crowding onset of a one-stream run (launch_policy.h crowd_kshift): floor(log2(n_steps / 2)) + 2."""
    per = max(g.n_steps // 2, 1)
    return per.bit_length() - 1 + 2
