"""Test-side restatements for the device quality read-outs (K7): the per-pair formula of calculate_layout_stress
(sgd.rs:1252-1275, Layout::distance) and the pass of measure_layout_quality.rs:100-208, written without the product's
quality.py.  The sum over dimensions is an explicit left-to-right loop, as the reference's is."""
import math

import numpy as np

NO_NODE = 0xFFFFFFFF


def plus_end(g, coords, dims):
    """(n_nodes, D) array of the coordinates the formula reads: x itself (dims = 0) or the + end of Layout.coords."""
    c = np.asarray(coords, dtype=np.float64)
    return c.reshape(g.n_nodes, 1) if dims == 0 else c.reshape(g.n_nodes, 2, dims)[:, 0, :]


def np_pairs_at(g, z):
    """All (s, s + z) inside one path."""
    S = g.n_steps
    if z >= S:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    first = g.path_first_step.astype(np.int64)
    path_of = np.repeat(np.arange(g.n_paths), np.diff(first))
    sa = np.arange(0, S - z, dtype=np.int64)
    sa = sa[path_of[sa] == path_of[sa + z]]
    return sa, sa + z


def np_pair_values(g, coords, dims, sa, sb):
    """(err, rel_sq, counted mask) of the pairs (sa[i], sb[i])."""
    pos, _ = g.step_positions()
    sn = g.step_node.astype(np.int64)
    d = np.abs(pos[sa].astype(np.float64) - pos[sb].astype(np.float64))
    ia, ib = sn[sa], sn[sb]
    ok = (d != 0.0) & (ia != NO_NODE) & (ib != NO_NODE)
    ia, ib, d = ia[ok], ib[ok], d[ok]
    c = plus_end(g, coords, dims)
    ss = np.zeros(d.shape[0], dtype=np.float64)
    for k in range(c.shape[1]):                                   # left to right, one rounding per operation
        delta = c[ia, k] - c[ib, k]
        ss = ss + delta * delta
    err = np.sqrt(ss) - d
    return err, (err * err) / (d * d), ok


def np_pair_errors(g, coords, dims, z):
    """dict(pairs, sum_rel_sq, max_rel_sq, sum_abs, sum_sq) over all pairs of steps z apart."""
    sa, sb = np_pairs_at(g, int(z))
    err, rel, _ = np_pair_values(g, coords, dims, sa, sb)
    return dict(pairs=int(err.shape[0]), sum_rel_sq=float(rel.sum()), max_rel_sq=float(rel.max()) if rel.size else 0.0,
                sum_abs=float(np.abs(err).sum()), sum_sq=float((err * err).sum()))


def py_stress_of_pairs(g, coords, dims, sa, sb):
    """calculate_layout_stress' loop body (sgd.rs:1252-1282) over the given candidate pairs, in plain Python floats, summed
    in order."""
    pos, _ = g.step_positions()
    pos = [int(v) for v in pos]
    sn = [int(v) for v in g.step_node]
    c = [[float(v) for v in row] for row in plus_end(g, coords, dims)]
    total, count = 0.0, 0
    for a, b in zip([int(v) for v in sa], [int(v) for v in sb]):
        path_dist = abs(float(pos[a]) - float(pos[b]))
        if path_dist == 0.0:
            continue
        ia, ib = sn[a], sn[b]
        if ia == NO_NODE or ib == NO_NODE:
            continue
        sum_sq = 0.0
        for ca, cb in zip(c[ia], c[ib]):
            delta = ca - cb
            sum_sq += delta * delta
        err = math.sqrt(sum_sq) - path_dist
        total += (err * err) / (path_dist * path_dist)
        count += 1
    return (math.sqrt(total / count) if count else 0.0), count


def np_sort_quality(g, order):
    """measure_layout_quality.rs:100-208 in int64: dict(steps, abs_err_sum, genomic_sum, sq_err_sum)."""
    order = np.asarray(order, dtype=np.int64)
    n = g.n_nodes
    node_len = g.node_len.astype(np.int64)
    spos = np.zeros(n, dtype=np.int64)
    spos[order] = np.concatenate([[0], np.cumsum(node_len[order])[:-1]])
    sa, sb = np_pairs_at(g, 1)
    sn = g.step_node.astype(np.int64)
    na, nb = sn[sa], sn[sb]
    ok = na != NO_NODE
    na, nb = na[ok], nb[ok]
    gd = node_len[na]
    pb = np.where(nb == NO_NODE, 0, spos[np.minimum(nb, n - 1)])
    ae = np.abs(np.abs(pb - spos[na]) - gd)
    return dict(steps=int(ae.shape[0]), abs_err_sum=int(ae.sum()), genomic_sum=int(gd.sum()),
                sq_err_sum=float((ae.astype(np.float64) ** 2).sum()))


def noisy_start(g, dims, seed, scale=3.0):
    """The reference's start (bp prefix sums; the layout's dimension 0, zeros elsewhere) plus seeded Gaussian noise."""
    rng = np.random.default_rng(seed)
    csum = np.concatenate([[0], np.cumsum(g.node_len.astype(np.int64))]).astype(np.float64)
    if dims == 0:
        return csum[:-1] + rng.normal(0.0, scale, g.n_nodes)
    c = np.zeros((g.n_nodes, 2, dims), dtype=np.float64)
    c[:, 0, 0], c[:, 1, 0] = csum[:-1], csum[1:]
    return np.ascontiguousarray((c + rng.normal(0.0, scale, c.shape)).reshape(-1))
