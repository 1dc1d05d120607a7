"""The items of the batch that tests/test_gpu_batch_sort_quality.py reads with gfs_batch_sort_quality (K7k), and the serial
restatements of what one workgroup of its first kernel does after the sort.  tests/test_batch_sort_quality_host.py holds the
generators to the seams they are meant to reach, without a device."""
import numpy as np

from util import G, load, graph_from_paths, absent_node_graph
from quality_restatement import seam_graph

SEGMENT_SORT_CAP = 8192
NAMES = ("simple", "lil", "DRB1", "chain64", "chain65", "chain1025", "chain2049", "one_node", "one_step", "absent_node", "medium")


def chain(n, seed):
    """One path over n nodes of lengths 1..16, whose S lines come in another order than the path visits them."""
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


_graphs = None


def graphs():
    """By NAMES.  Made once and only read."""
    global _graphs
    if _graphs is None:
        _graphs = [load("simple.gfa"), load("lil.gfa"), load("DRB1-3123.gfa"), chain(64, 3), chain(65, 4), chain(1025, 5), chain(2049, 6),
                   graph_from_paths([[0, 0, 0]], [5]),                    # one node, stepped on three times
                   graph_from_paths([[1]], [3, 4, 5]),                    # a path, but fewer than two steps
                   absent_node_graph(), seam_graph("medium")]
    return _graphs


def segment_padded(n):
    p = 64
    while p < n:
        p <<= 1
    return p


def segment_block(padded):
    return min(max(padded // 2, 64), 1024)


def launch_order(n_nodes, cap):
    """batch_readout_plan.h segment_launch_order, restated: (order, rows within the cap)."""
    key = [segment_padded(n) if n <= cap else 1 << 62 for n in n_nodes]
    order = sorted(range(len(n_nodes)), key=lambda i: key[i])            # (sorted is stable)
    return order, sum(k < 1 << 62 for k in key)


def block_scan_scatter(lens_by_rank, index, perm, block):
    """What a workgroup of `block` threads does after its sort: the exclusive scan of the node lengths in rank order, in chunks of
    one block — an inclusive scan per wave of 64 (Hillis-Steele), the waves' totals added in wave order, the running sum carried
    from chunk to chunk — and spos[perm[index[r]]] = prefix[r].  Returns (spos by slot, total), uint64."""
    n = len(lens_by_rank)
    spos = np.zeros(n, dtype=np.uint64)
    carry = np.uint64(0)
    for base in range(0, n, block):
        chunk = np.zeros(block, dtype=np.uint64)
        live = min(block, n - base)
        chunk[:live] = lens_by_rank[base:base + live]
        incl = chunk.reshape(block // 64, 64).copy()
        d = 1
        while d < 64:
            up = np.zeros_like(incl)
            up[:, d:] = incl[:, :-d]
            incl = incl + up
            d <<= 1
        wave_total = incl[:, 63]
        before = np.concatenate([[np.uint64(0)], np.cumsum(wave_total, dtype=np.uint64)[:-1]])
        excl = (incl + before[:, None] - chunk.reshape(block // 64, 64)).reshape(-1)
        r = np.arange(base, base + live)
        spos[perm[index[r]]] = carry + excl[:live]
        carry = carry + wave_total.sum(dtype=np.uint64)
    return spos, int(carry)
