"""Test-side restatements for the device quality read-outs (K7): the per-pair formula of calculate_layout_stress
(sgd.rs:1252-1275, Layout::distance) and the pass of measure_layout_quality.rs:100-208, written without the product's
quality.py.  The sum over dimensions is an explicit left-to-right loop, as the reference's is.

Also here, written from the project's own headers and DESIGN.md (no constant is imported from the product):
  - the fixed tree in which K7a, K7g and K7c take their double sums (thread_sums -> block_partials -> grid_total; tree_sum),
    a function of n_steps alone, so that a test can hold those sums to the device's bit for bit;
  - the tile decomposition of K7d's integer fields (tile_counts, path_counts_from_tiles);
  - grouped(): the per-pair values grouped per path and per node and listed in step order (K7d, K7e, K7f);
  - the seam graphs of tests/test_gpu_readout_seams.py (seam_graph) and shuffled_start.
The tree and the tile functions take the faults that tests/test_readout_seams_host.py injects as arguments that default to
"none"."""
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


def shuffled_start(g, dims, seed):
    """The reference's start positions handed to the nodes in a seeded random order."""
    perm = np.random.default_rng(seed).permutation(g.n_nodes)
    start = noisy_start(g, dims, 0, scale=0.0)
    if dims == 0:
        return np.ascontiguousarray(start[perm])
    return np.ascontiguousarray(start.reshape(g.n_nodes, 2 * dims)[perm].reshape(-1))


def path_of_step(g):
    first = g.path_first_step.astype(np.int64)
    return np.repeat(np.arange(g.n_paths), np.diff(first))


# ---- the fixed reduction tree of K7a, K7g and K7c (quality_device.h, batch_readout_plan.h) ------------------
Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS = 256, 8, 2048
Q_TILE, Q_COMBINE_LOAD = 512, 64                                  # K7d / K7e: steps per tile; tiles per load of the combine


def quality_blocks_of(n_steps):
    """Workgroups of a step pass: ceil(n_steps / 2048), at least 1, at most 2048."""
    per_block = Q_BLOCK * Q_PAIRS_PER_THREAD
    return min(max(-(-int(n_steps) // per_block), 1), Q_MAX_BLOCKS)


def uncapped_blocks_of(n_steps):
    """The same without the cap: what a stride must NOT be taken from (an injected fault)."""
    return max(-(-int(n_steps) // (Q_BLOCK * Q_PAIRS_PER_THREAD)), 1)


def thread_sums(values, counted, n_steps, stride_blocks=None):
    """values[s], counted[s] for s in [0, n_steps - z).  Thread (b, t) of B = quality_blocks_of(n_steps) workgroups starts at
    b * 256 + t and strides by B * 256; it adds the counted values in order onto +0.0, a skipped pair leaves it alone.
    Returns float64[B * 256].  stride_blocks: the grid the stride is taken from (default: the grid itself)."""
    values = np.asarray(values, dtype=np.float64)
    counted = np.asarray(counted, dtype=bool)
    threads = quality_blocks_of(n_steps) * Q_BLOCK
    stride = (quality_blocks_of(n_steps) if stride_blocks is None else int(stride_blocks)) * Q_BLOCK
    assert stride >= threads and values.shape == counted.shape and values.ndim == 1
    n = values.shape[0]
    rounds = -(-n // stride) if n else 0
    v = np.zeros(rounds * stride, dtype=np.float64)
    m = np.zeros(rounds * stride, dtype=bool)
    v[:n], m[:n] = values, counted
    v, m = v.reshape(rounds, stride)[:, :threads], m.reshape(rounds, stride)[:, :threads]
    acc = np.zeros(threads, dtype=np.float64)
    for r in range(rounds):
        acc = np.where(m[r], acc + v[r], acc)
    return acc


def block_partials(acc):
    """The wave: v = v + v[lane ^ off] for off = 32, 16, 8, 4, 2, 1, then lane 0.  The workgroup: ((w0 + w1) + w2) + w3."""
    a = acc.reshape(-1, Q_BLOCK // 64, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ off]
    w = a[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def grid_total(partials, staged=None):
    """From +0.0, the workgroups' partials in workgroup order.  staged: how many partials the reduce reads (default: all)."""
    total = 0.0
    for v in partials[:staged].tolist():
        total = total + v
    return total


def tree_sum(values, counted, n_steps, stride_blocks=None, staged=None):
    return grid_total(block_partials(thread_sums(values, counted, n_steps, stride_blocks)), staged)


def tree_count(counted, n_steps, stride_blocks=None, staged=None):
    """`pairs` in the same decomposition: a count, whatever the order — unless a fault leaves pairs or partials out."""
    ones = np.ones(np.asarray(counted).shape[0], dtype=np.float64)
    return int(tree_sum(ones, counted, n_steps, stride_blocks, staged))      # (exact: < 2^53)


def step_values(g, coords, dims, z):
    """The per-pair values of K7a in STEP order: dict(counted, rel, abs, sq), each of length max(n_steps - z, 0); entries of
    pairs that are not counted are 0."""
    n = max(g.n_steps - int(z), 0)
    sa, sb = np_pairs_at(g, int(z))
    err, rel, ok = np_pair_values(g, coords, dims, sa, sb)
    at = sa[ok]
    out = dict(counted=np.zeros(n, dtype=bool), rel=np.zeros(n), abs=np.zeros(n), sq=np.zeros(n))
    out["counted"][at] = True
    out["rel"][at], out["abs"][at], out["sq"][at] = rel, np.abs(err), err * err
    return out


def tree_pair_errors(g, coords, dims, z, stride_blocks=None, staged=None):
    """K7a's row for step distance z, the sums in the device's tree: dict(pairs, sum_rel_sq, max_rel_sq, sum_abs, sum_sq)."""
    v = step_values(g, coords, dims, z)
    c, S = v["counted"], g.n_steps
    kw = dict(stride_blocks=stride_blocks, staged=staged)
    return dict(pairs=tree_count(c, S, **kw), sum_rel_sq=tree_sum(v["rel"], c, S, **kw),
                max_rel_sq=float(v["rel"].max()) if v["rel"].size else 0.0,
                sum_abs=tree_sum(v["abs"], c, S, **kw), sum_sq=tree_sum(v["sq"], c, S, **kw))


def sort_step_values(g, order):
    """K7c per adjacent step pair (s, s + 1) in step order: (abs_err int64[n_steps - 1], counted).  Counted: both steps on one
    path and the first on a node; an absent second node stands at position 0."""
    order = np.asarray(order, dtype=np.int64)
    n = g.n_nodes
    node_len = g.node_len.astype(np.int64)
    spos = np.zeros(n, dtype=np.int64)
    spos[order] = np.concatenate([[0], np.cumsum(node_len[order])[:-1]])
    sn = g.step_node.astype(np.int64)
    pth = path_of_step(g)
    na, nb = sn[:-1], sn[1:]
    counted = (pth[:-1] == pth[1:]) & (na != NO_NODE)
    pa = spos[np.minimum(na, n - 1)]
    pb = np.where(nb == NO_NODE, 0, spos[np.minimum(nb, n - 1)])
    gd = node_len[np.minimum(na, n - 1)]
    ae = np.abs(np.abs(pb - pa) - gd)
    return np.where(counted, ae, 0), counted


# ---- K7d's tiles, integer fields only (quality_kernels.hip path_tiles_kernel / path_combine_kernel) ---------------------------
def tile_counts(g, flag):
    """Per tile of Q_TILE steps: (head, tail) = how many steps with flag[s] the tile holds on the path of its FIRST step and on
    the path of its LAST step.  flag = all ones gives `steps`, the counted mask of a step distance gives `pairs`."""
    S = g.n_steps
    flag = np.asarray(flag, dtype=np.int64)
    pth = path_of_step(g)
    tile = np.arange(S) // Q_TILE
    n_tiles = -(-S // Q_TILE)
    lo = np.arange(n_tiles) * Q_TILE
    hi = np.minimum(lo + Q_TILE, S)
    head = np.bincount(tile, weights=flag * (pth == pth[lo][tile]), minlength=n_tiles).astype(np.int64)
    tail = np.bincount(tile, weights=flag * (pth == pth[hi - 1][tile]), minlength=n_tiles).astype(np.int64)
    return head, tail


def path_counts_from_tiles(g, flag, max_tiles=None, swap_at_first_tile=False):
    """A per-path count the way K7d takes it: a path inside one tile is counted by the tile pass; a longer one is the sum of
    its tiles' partials in tile order, the TAIL partial in its first tile where it starts inside that tile and HEAD partials
    everywhere else.  Also returns the loads of Q_COMBINE_LOAD tiles the combine takes per path (0: no combine).
    Faults: max_tiles = 64 drops a path's tiles past the 64th; swap_at_first_tile takes head for tail and tail for head there."""
    head, tail = tile_counts(g, flag)
    first = g.path_first_step.astype(np.int64)
    flag = np.asarray(flag, dtype=np.int64)
    csum = np.concatenate([[0], np.cumsum(flag)])
    out = csum[first[1:]] - csum[first[:-1]]                       # the tile pass' own results
    loads = np.zeros(g.n_paths, dtype=np.int64)
    cnt = np.diff(first)
    for p in np.flatnonzero(cnt > 0).tolist():
        b = int(first[p])
        tb, te = b // Q_TILE, (b + int(cnt[p]) - 1) // Q_TILE
        if tb == te:
            continue
        loads[p] = -(-(te - tb + 1) // Q_COMBINE_LOAD)
        last = te if max_tiles is None else min(te, tb + max_tiles - 1)
        use_tail = (b % Q_TILE != 0) != bool(swap_at_first_tile)
        total = int(tail[tb] if use_tail else head[tb])
        total += int(head[tb + 1:last + 1].sum())
        out[p] = total
    return out, loads


# ---- K7d, K7e, K7f: the per-pair values grouped ---------------------------------------------------------------------------------
PATH_ERROR_DTYPE = np.dtype([("steps", "<u8"), ("reverse_steps", "<u8"), ("pairs", "<u8"), ("sum_rel_sq", "<f8"), ("max_rel_sq", "<f8"),
                             ("sum_abs", "<f8"), ("sum_sq", "<f8"), ("stretched", "<u8")])
STRETCHED_PAIR_DTYPE = np.dtype([("step_a", "<u8"), ("step_b", "<u8"), ("path", "<u8"), ("d_path", "<f8"), ("d_layout", "<f8")])
NODE_ERROR_DTYPE = np.dtype([("pairs", "<u8"), ("stretched", "<u8"), ("max_rel_sq", "<f8")])


def grouped(g, coords, dims, z, ratio):
    """dict(paths, nodes, list, counted): the restatement's per-pair values at step distance z grouped per path (K7d) and per
    node (K7f), and the stretched pairs in ascending step order (K7e).  d_layout = err + d_path; a counted pair is stretched
    when d_layout / d_path > ratio."""
    sa, sb = np_pairs_at(g, z)
    err, rel, ok = np_pair_values(g, coords, dims, sa, sb)
    sa, sb = sa[ok], sb[ok]
    pos, _ = g.step_positions()
    d_path = np.abs(pos[sa].astype(np.float64) - pos[sb].astype(np.float64))
    d_layout = err + d_path
    stretched = d_layout / d_path > ratio
    first = g.path_first_step.astype(np.int64)
    path_of = np.repeat(np.arange(g.n_paths), np.diff(first))
    pa = path_of[sa]
    paths = np.zeros(g.n_paths, dtype=PATH_ERROR_DTYPE)
    paths["steps"] = np.diff(first)
    paths["reverse_steps"] = np.bincount(path_of[g.step_is_rev.astype(bool)], minlength=g.n_paths)
    paths["pairs"] = np.bincount(pa, minlength=g.n_paths)
    paths["stretched"] = np.bincount(pa[stretched], minlength=g.n_paths)
    np.maximum.at(paths["max_rel_sq"], pa, rel)
    for k, v in (("sum_rel_sq", rel), ("sum_abs", np.abs(err)), ("sum_sq", err * err)):
        paths[k] = np.bincount(pa, weights=v, minlength=g.n_paths)
    sn = g.step_node.astype(np.int64)
    na, nb = sn[sa], sn[sb]
    other = nb != na                                                    # a pair from a node to itself counts once
    nodes = np.zeros(g.n_nodes, dtype=NODE_ERROR_DTYPE)
    nodes["pairs"] = np.bincount(na, minlength=g.n_nodes) + np.bincount(nb[other], minlength=g.n_nodes)
    nodes["stretched"] = np.bincount(na[stretched], minlength=g.n_nodes) + np.bincount(nb[other & stretched], minlength=g.n_nodes)
    np.maximum.at(nodes["max_rel_sq"], na, rel)
    np.maximum.at(nodes["max_rel_sq"], nb, rel)
    lst = np.zeros(int(stretched.sum()), dtype=STRETCHED_PAIR_DTYPE)
    lst["step_a"], lst["step_b"], lst["path"] = sa[stretched], sb[stretched], pa[stretched]
    lst["d_path"], lst["d_layout"] = d_path[stretched], d_layout[stretched]
    assert np.all(np.diff(lst["step_a"].astype(np.int64)) > 0)
    return dict(paths=paths, nodes=nodes, list=lst, counted=int(sa.shape[0]))


_expected = {}


def expected(g, name, dims, kind, coords, z, ratio):
    """grouped() of the named case — computed once per case and shared; nobody changes what it returns."""
    key = (name, dims, kind, z, ratio)
    if key not in _expected:
        _expected[key] = grouped(g, coords, dims, z, ratio)
    return _expected[key]


# ---- the seam graphs (tests/test_gpu_readout_seams.py; their conditions: tests/test_readout_seams_host.py) ---------------------
SEAM_STEPS = {"medium": 524288 + 1000, "medium-256": 524288, "large": 4194304 + 70000}
SEAM_NODES = {"medium": 20000, "medium-256": 20000, "large": 300000}


def seam_graph(name):
    """Seeded synthetic graphs whose sizes lie just past the seams of the read-out kernels.  Node lengths 0..8 (d_path == 0
    occurs), 30 % of the steps reverse, about one step in 500 absent (NO_NODE).  Long paths walk the nodes upwards from a random
    start, short ones visit random nodes.  Paths in step order:
      medium / medium-256: 32 768 steps from step 0 (64 tiles, one load of the combine); 65 tiles from a tile boundary; 3 000
        paths of 2-5 steps; 130 tiles and more from inside a tile; one path without steps; paths of 30 000-40 000 steps up to the
        total; one path of 12 absent steps at the end.
      large: paths of 150 000-200 000 steps, then 5 000 paths of 2-5 steps, then one last path up to the total."""
    from gfasort_amd import graph as G
    total, n_nodes = SEAM_STEPS[name], SEAM_NODES[name]
    rng = np.random.default_rng(sorted(SEAM_STEPS).index(name) + 41)
    if name == "large":
        shorts = rng.integers(2, 6, 5000).tolist()
        lens = []
        while total - sum(shorts) - sum(lens) > 200000:
            lens.append(int(rng.integers(150000, 200001)))
        lens += shorts
    else:
        lens = [64 * Q_TILE, 64 * Q_TILE + 100] + rng.integers(2, 6, 3000).tolist()
        if sum(lens) % Q_TILE == 0:
            lens.append(3)
        lens += [130 * Q_TILE + 7, 0]
        while total - 12 - sum(lens) > 45000:
            lens.append(int(rng.integers(30000, 40001)))
        lens += [total - 12 - sum(lens), 12]
    if name == "large":
        lens.append(total - sum(lens))
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.min() >= 0 and int(lens.sum()) == total
    first = np.concatenate([[0], np.cumsum(lens)])
    pth = np.repeat(np.arange(lens.shape[0]), lens)
    local = np.arange(total) - first[pth]
    walk = (rng.integers(0, n_nodes, lens.shape[0])[pth] + local) % n_nodes
    step_node = np.where(lens[pth] <= 5, rng.integers(0, n_nodes, total), walk).astype(np.uint32)
    step_node[rng.random(total) < 0.002] = NO_NODE
    if name != "large":
        step_node[first[-2]:] = NO_NODE
    return G.FlatGraph(node_len=rng.integers(0, 9, n_nodes).astype(np.uint32), step_node=step_node,
                       step_is_rev=(rng.random(total) < 0.3).astype(np.uint8), path_first_step=first.astype(np.uint64),
                       node_ids=np.arange(1, n_nodes + 1, dtype=np.uint64), path_names=[f"p{i}" for i in range(lens.shape[0])])
