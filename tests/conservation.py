"""The one exact statement about a racy full-width SGD run: every term adds -r_d to one word and +r_d to another, so the sum
of a dimension over a connected component changes only by rounding, and a word that no term names does not change at all.
guarded_graph() is the small graph every case runs on, check() the assertion.  No GPU here: test_conservation_host.py runs the
oracle through it, test_gpu_conservation.py every full-width kernel."""
import math

import numpy as np

from util import G, graph_from_paths

NO_NODE = G.NO_NODE
N_A, N_B, N_SENTINELS = 6000, 2000, 500


def no_repeat_inside_a_path(g):
    """No path steps on a node twice (the predicate of test_gpu_layout_reference_streams.py): no term has i == j, so every
    update is two adds to two different nodes."""
    first = g.path_first_step.astype(np.int64)
    path_of = np.repeat(np.arange(first.shape[0] - 1), np.diff(first))
    present = g.step_node != NO_NODE
    key = path_of[present] * (g.n_nodes + 1) + g.step_node[present].astype(np.int64)
    return np.unique(key).shape[0] == key.shape[0]


def guarded_graph():
    """(g, node_perm).  8500 nodes, dense indices of the three parts interleaved by a seeded permutation:
    A  the chain of test_gpu_pool_walk.py: 6000 nodes of lengths 1..16, one path over all of it and five over overlapping
       stretches of 1500 to 3000 steps;
    B  a second chain of 2000 nodes with a path over all of it and one over 1300 of its steps, no node shared with A;
    500 sentinel nodes that no path visits.
    Twelve steps on absent nodes (NO_NODE) are spliced into three of the paths, one step in eight is reverse, no path steps on
    a node twice, and the shortest path has 1300 steps (>= 4 * 64: GFS_F_BUNDLE(64) is a sensible request).
    g.components = {"A": dense indices, "B": dense indices}, g.sentinels = dense indices.
    node_perm[k] = slot of dense node k (hip.Context(g, node_perm=...)): a seeded random permutation with a sentinel in slot 0,
    a sentinel in slot n - 1 and the rest scattered among the visited slots, so that an add to a neighbouring slot or a
    neighbouring plane lands on a sentinel or in the other component more often than not."""
    n = N_A + N_B + N_SENTINELS
    lens_a = np.random.default_rng(11).integers(1, 17, N_A)                    # test_gpu_pool_walk.py _graph()
    rng = np.random.default_rng(13)
    dense = rng.permutation(n)
    a, b, sentinels = dense[:N_A], dense[N_A:N_A + N_B], np.sort(dense[N_A + N_B:])
    paths = [a.tolist()] + [a[s:s + w].tolist() for s, w in ((0, 3000), (1000, 2500), (2500, 3000), (4000, 1500), (300, 2000))]
    paths += [b.tolist(), b[500:1800].tolist()]
    for pth, at in ((0, (7, 2999, 3000, 5990)), (3, (0, 1, 1500, 2990)), (6, (63, 64, 1000, 1999))):
        for k in sorted(at, reverse=True):                                     # absent nodes: at a path's start, in a row, mid-run
            paths[pth].insert(k, NO_NODE)
    node_len = np.zeros(n, dtype=np.uint32)
    node_len[a], node_len[b], node_len[sentinels] = lens_a, rng.integers(1, 17, N_B), rng.integers(1, 17, N_SENTINELS)
    n_steps = sum(len(p) for p in paths)
    g = graph_from_paths(paths, node_len, rev=(rng.random(n_steps) < 0.125).astype(np.uint8))
    g.components = {"A": np.sort(a), "B": np.sort(b)}
    g.sentinels = sentinels
    assert no_repeat_inside_a_path(g)
    assert int((g.step_node == NO_NODE).sum()) == 12 and int(g.step_is_rev.sum()) >= 1
    assert min(len(p) for p in paths) >= 4 * 64
    visited = np.zeros(n, dtype=bool)
    visited[g.step_node[g.step_node != NO_NODE]] = True
    assert not visited[sentinels].any() and visited.sum() == N_A + N_B
    perm = rng.permutation(n).astype(np.uint32)
    for slot, s in ((0, sentinels[0]), (n - 1, sentinels[1])):                 # swap a sentinel into each end slot
        holder = int(np.flatnonzero(perm == slot)[0])
        perm[holder], perm[s] = perm[s], slot
    assert np.array_equal(np.sort(perm), np.arange(n)) and not visited[perm == 0].any() and not visited[perm == n - 1].any()
    return g, perm


def longest_path_bp(g):
    present = g.step_node != NO_NODE
    bp = np.where(present, g.node_len[np.where(present, g.step_node, 0)], 0).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(bp)])
    first = g.path_first_step.astype(np.int64)
    return float((csum[first[1:]] - csum[first[:-1]]).max())


def check(before, after, g, dims, updates, case=""):
    """before, after: positions (dims == 0: x[n_nodes]) or coordinates (Layout order, c[(2 * node + end) * dims + k]) around
    `updates` term updates.  Asserts, for g.components and g.sentinels (a graph without them is one component, no sentinels):

    Sentinels.  Every word of every sentinel node is bit-identical (uint64 views).

    Conservation.  For every component c and dimension k, drift = |fsum(after_k, -before_k)| over the component's words — ONE
    exact sum of the differences (math.fsum), not the difference of two rounded sums — is at most

        bound = 3 * U * 2^-53 * M,   U = updates,   M = max(largest |word| of c, k before or after, longest path in bp).

    Derivation.  An update is -r to one word and +r to another: in exact arithmetic the sum stays.  What the hardware adds to
    it is rounding: a correctly rounded operation with result v errs by at most 2^-53 |v|.  An update costs at most two memory
    adds, whose results are coordinates, |v| <= M.  The fused, twin and merged trips add two moves in a register first
    (-r + r', -(r + r')) and issue ONE memory add for them: at most one register add per update, and every register add
    saves a memory add.  |r| <= max(|dx|, d_ij) / 2 (mu <= 1: a term moves each end at most half of the longer of where it
    is and where it should be), so a register sum is at most max(2 M_coord, longest path): with m <= U register adds the
    total is (2U - m) M_coord + m max(2 M_coord, L) <= 3 U max(M_coord, L).  Hence the 3 and the path length in M.  U is the
    whole run's count for every component (the share of each is not known): that only loosens the bound, by less than the
    number of components.  Premise: the values a word passes through stay within M.  The oracle's own drift is four orders of
    magnitude inside the bound (test_conservation_host.py prints it: ~2e-9 against ~2e-5 bp at 1e6 updates); one lost, doubled
    or misplaced add of a move above the bound breaks it.

    Movement.  Every component moved.

    Prints and returns one row (case, component, k, drift, bound, drift / bound) per conservation assertion."""
    before = np.ascontiguousarray(before, dtype=np.float64).reshape(-1)
    after = np.ascontiguousarray(after, dtype=np.float64).reshape(-1)
    D = max(int(dims), 1)
    words = (1 if dims == 0 else 2) * D                                        # per node
    assert before.shape == after.shape == (g.n_nodes * words,)
    assert np.isfinite(after).all(), case
    b, a = before.reshape(g.n_nodes, words), after.reshape(g.n_nodes, words)
    components = getattr(g, "components", None) or {"all": np.arange(g.n_nodes)}
    sentinels = getattr(g, "sentinels", np.zeros(0, dtype=np.int64))
    touched = np.flatnonzero((a[sentinels].view(np.uint64) != b[sentinels].view(np.uint64)).any(axis=1))
    assert touched.shape[0] == 0, (case, "sentinel nodes written", sentinels[touched][:8].tolist(), int(touched.shape[0]))
    L = longest_path_bp(g)
    rows, failed = [], []
    for name, nodes in components.items():
        assert not np.array_equal(a[nodes], b[nodes]), (case, name, "did not move")
        for k in range(D):
            ak, bk = a[nodes][:, k::D].reshape(-1), b[nodes][:, k::D].reshape(-1)
            drift = abs(math.fsum(ak.tolist() + (-bk).tolist()))
            M = max(float(np.abs(ak).max()), float(np.abs(bk).max()), L)
            bound = 3.0 * updates * 2.0 ** -53 * M
            rows.append((case, name, k, drift, bound, drift / bound))
            print(f"conservation {case} {name} k={k}: drift {drift:.3e} bound {bound:.3e} drift/bound {drift / bound:.2e}")
            if not drift <= bound:
                failed.append(rows[-1])
    assert not failed, failed
    return rows
