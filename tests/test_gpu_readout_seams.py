"""The quality read-outs (K6, K7a-K7g) past the first trip of their loops, on graphs just large enough to get there.  Positions
are uploaded and measured; no SGD is run.  The graphs are quality_restatement.seam_graph's, and tests/test_readout_seams_host.py
asserts from the graphs themselves that they reach each seam below and that each comparison made here fails on the fault it
is there for.

Which test reaches which loop, and which assertion shows that it did:

| code                                             | reached by                                   | shown by |
| reduce_partials_kernel, second staging tile      | K7a on `medium` (257 workgroups: a full tile | `pairs` is exact and the three sums are the restated tree's bit for bit: a
|   of partials, partial last tile                 |   and a tile of ONE entry); `medium-256`     |   reduce that stops after 256 partials loses workgroup 256's pairs (host
|                                                  |   (exactly one full tile) beside it          |   file: every one of the four figures changes; on `medium-256` none does)
| batch_reduce_partials_kernel, the same loop      | K7g: batch [DRB1, medium, lil]               | medium's rows are its own context's bytes, which the K7a test of this file
|                                                  |   (medium's first_block is 18, not 0)        |   holds to the tree
| quality_blocks_of capped at 2048 (K7a, K7c, K7f, | K7a, K7c, K7f on `large` (4 264 304 steps:   | `pairs` / `steps` / the per-node counts are exact: a stride from the uncapped
|   K7g step passes): 9 pairs per thread, stride   |   69 999 threads take 9 pairs, the rest 8)   |   grid (2083 x 256) skips 8 960 pairs per pass; the sums bit for bit: the
|   of the capped grid                             |                                              |   tree is built on 2048 workgroups
| path_combine_kernel, more than 64 tiles          | K7d on `medium`: paths of 64 tiles (one      | steps, reverse steps, pairs, stretched and max_rel_sq per path are exact: a
|                                                  |   load), 65 from a tile boundary (the second |   combine that stops after 64 tiles loses the steps of the rest, one that takes
|                                                  |   load has one tile), 130 from inside a tile |   head for tail at the first tile counts another path's steps; the test
|                                                  |   (tail partial first, three loads)          |   prints and asserts how many paths took 1, 2 and >= 3 loads
| pair_list_kernel, grid stride                    | K7b: 600 000 listed pairs on `medium`        | every rel_sq is np_pair_values' bit for bit, -1 where skipped, in all 600 000
|                                                  |   (2048 x 256 threads = 524 288)             |   places; without the stride the entries past 524 288 are whatever the scratch held
| scatter_sorted_pos_kernel, sort_keys_kernel,     | K6, K7c, K7f on `large` (300 000 nodes,      | the order is numpy's stable argsort over all nodes; K7c's integer sums are
|   gather_node_errors_kernel: 1024 x 256 threads; |   262 144 threads)                           |   exact (a node without a sorted position stands at 0); K7f's rows are exact
|   rocPRIM scan and sort over > 1 block of nodes  |                                              |   for every node, also those past 262 144
| stretched_tiles_kernel + rocPRIM scan, thousands | K7e on `medium` (1 026 tiles) and `large`    | the total and the list are exact field by field at cap = total, total - 1,
|   of tiles; offset >= cap skips                  |   (8 329 tiles), most pairs stretched        |   1000 and 0; entries past the list keep the sentinel

The double sums.  K7a, K7g and K7c promise a fixed tree that is a function of n_steps alone; it is restated
in quality_restatement.py (thread_sums, block_partials, grid_total) and compared bit for bit.  Beside it stays the order-free
bound of test_gpu_quality_readout.py — n * 2^-52 relative against numpy's own sum — so that a failure of the first alone says
"the order differs" and a failure of both says "a value differs".  Where the bits differ the message names how many per-pair
values (read through K7b) differ from the restatement's.  K7d's per-path sums keep the bound (pairs * 2^-52); its segmented scan
is not restated.

Every test prints one line `seam-table | case | n_steps | workgroups | tiles | pairs | seconds` (profiles/r14)."""
import time

import numpy as np
import pytest

from util import P, load, NO_NODE
from gfasort_amd import hip
from gfasort_amd.distributed import subgraph
import quality_restatement as R
from quality_restatement import (seam_graph, noisy_start, shuffled_start, step_values, tree_sum, tree_count, np_pair_values,
                                 np_pair_errors, np_sort_quality, sort_step_values, grouped, path_counts_from_tiles, path_of_step,
                                 quality_blocks_of, Q_TILE)

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SUMS = ("sum_rel_sq", "sum_abs", "sum_sq")
STEP_VALUE_OF = {"sum_rel_sq": "rel", "sum_abs": "abs", "sum_sq": "sq"}
ZS = {"medium": [1, 64, 65, 1000], "medium-256": [1, 64, 65, 1000], "large": [1, 1000]}
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 7, -1.5, -2.5)

_cache = {}


def graph(name):
    if name not in _cache:
        _cache[name] = load("DRB1-3123.gfa") if name == "DRB1" else load("lil.gfa") if name == "lil" else seam_graph(name)
    return _cache[name]


def positions(name, dims, kind):
    """Seeded test positions, made once and only read."""
    key = (name, dims, kind)
    if key not in _cache:
        g = graph(name)
        x = noisy_start(g, dims, 17 + dims) if kind == "noisy" else shuffled_start(g, dims, 23 + dims)
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def _sane_space(p):
    """The derived space is the longest path in bp, and the zeta table has that many entries: cap it, no SGD is run here."""
    p.space = min(p.space, 20_000)
    return p


def context(g, dims, x, node_perm=None, cfg=None):
    ctx = hip.Context(g, node_perm=node_perm)
    p = _sane_space(P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd)
    p.iter_max = 2
    (ctx.setup_nd if dims else ctx.setup_1d)(p, cfg)
    ctx.upload(x)
    return ctx


def table_row(case, g, pairs, t0):
    print(f"seam-table | {case} | {g.n_steps} | {quality_blocks_of(g.n_steps)} | {-(-g.n_steps // Q_TILE)} | {int(pairs)} | "
          f"{time.perf_counter() - t0:.2f}")


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


# ---- the tree and the bound, once per (graph, dims, z) --------------------------------------------------------------------------
def k7a_wanted(name, dims, z):
    """dict(pairs, max_rel_sq, tree = the three sums in the device's tree, plain = numpy's own sums) of the noisy positions."""
    key = ("k7a", name, dims, z)
    if key not in _cache:
        g = graph(name)
        v = step_values(g, positions(name, dims, "noisy"), dims, z)
        c = v["counted"]
        _cache[key] = dict(pairs=tree_count(c, g.n_steps), max_rel_sq=float(v["rel"].max()),
                           tree={k: tree_sum(v[STEP_VALUE_OF[k]], c, g.n_steps) for k in SUMS},
                           plain={k: float(v[STEP_VALUE_OF[k]][c].sum()) for k in SUMS})
        assert _cache[key]["pairs"] == int(c.sum()) > 0
    return _cache[key]


def per_pair_differences(ctx, g, x, dims, z):
    """How many per-pair values, read through K7b, differ from the restatement's — for the message of a failed comparison."""
    sa = np.arange(0, g.n_steps - z, dtype=np.int64)
    same = path_of_step(g)[sa] == path_of_step(g)[sa + z]
    sa = sa[same]
    _, rel, ok = np_pair_values(g, x, dims, sa, sa + z)
    want = np.full(sa.shape[0], -1.0)
    want[ok] = rel
    got = ctx.stress_of_pairs(sa, sa + z)[2]
    bad = np.flatnonzero(bits(got) != bits(want))
    first = f"; first: pair ({sa[bad[0]]}, {sa[bad[0]] + z}) device {got[bad[0]]!r} restatement {want[bad[0]]!r}" if bad.size else ""
    return f"{bad.size} of {sa.shape[0]} per-pair rel_sq differ from the restatement{first}"


def assert_row_is_the_tree(ctx, name, dims, row):
    g, z = graph(name), int(row["step_distance"])
    want = k7a_wanted(name, dims, z)
    print(f"{name} dims={dims} z={z} pairs={int(row['pairs'])}/{want['pairs']}",
          *(f"{k}: {float(row[k])!r} tree {want['tree'][k]!r} numpy {want['plain'][k]!r}" for k in SUMS))
    assert int(row["pairs"]) == want["pairs"]
    assert float(row["max_rel_sq"]) == want["max_rel_sq"]
    for k in SUMS:
        if bits(row[k]) != bits(want["tree"][k]):
            raise AssertionError(f"{name} dims={dims} z={z} {k}: device {float(row[k])!r}, tree {want['tree'][k]!r}, numpy "
                                 f"{want['plain'][k]!r}; " + per_pair_differences(ctx, g, positions(name, dims, "noisy"), dims, z))
        assert abs(float(row[k]) - want["plain"][k]) <= want["pairs"] * U * abs(want["plain"][k]), (k, z)


# ---- K7a ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims", [("medium", 0), ("medium", 2), ("medium", 8), ("medium-256", 0), ("medium-256", 2),
                                       ("large", 0), ("large", 2)])
def test_pair_errors_are_the_restated_tree_bit_for_bit(name, dims):
    t0 = time.perf_counter()
    g, x, zs = graph(name), positions(name, dims, "noisy"), ZS[name]
    ctx = context(g, dims, x)
    rows = ctx.pair_errors(zs)
    assert rows["step_distance"].tolist() == zs
    for row in rows:
        assert_row_is_the_tree(ctx, name, dims, row)
    assert ctx.pair_errors(zs).tobytes() == rows.tobytes()               # a second call: identical bytes
    ctx.close()
    assert hip.pair_errors(g, x, zs, dims).tobytes() == rows.tobytes()   # the one-shot entry: identical bytes
    table_row(f"K7a {name} D={dims} z={zs}", g, rows["pairs"].sum(), t0)


# ---- K7b ------------------------------------------------------------------------------------------------------------------------
def listed_pairs(g, n=600_000, seed=77):
    """Seeded step pairs: mostly inside a path at a distance of 1..2000 steps; among them equal steps, pairs across paths,
    pairs on absent steps and pairs whose steps lie on zero-length nodes."""
    rng = np.random.default_rng(seed)
    S = g.n_steps
    sa = rng.integers(0, S, n)
    sb = np.minimum(sa + rng.integers(1, 2001, n), S - 1)
    sb[:20000] = sa[:20000]                                              # equal steps: d_path == 0
    sb[20000:60000] = rng.integers(0, S, 40000)                          # anywhere: across paths, nearly all
    absent = np.flatnonzero(g.step_node == NO_NODE)
    sa[60000:80000] = rng.choice(absent, 20000)
    sb[80000:100000] = rng.choice(absent, 20000)
    zero = np.flatnonzero((g.step_node != NO_NODE) & (g.node_len[np.minimum(g.step_node, g.n_nodes - 1)] == 0))
    zero = zero[zero + 1 < S]
    sa[100000:140000] = rng.choice(zero, 40000)                          # (s, s + 1) from a zero-length node: d_path == 0
    sb[100000:140000] = sa[100000:140000] + 1
    back = slice(140000, 200000)                                         # the later step first
    sa[back], sb[back] = sb[back].copy(), sa[back].copy()
    return sa.astype(np.uint64), sb.astype(np.uint64)


@pytest.mark.parametrize("dims", [0, 2, 8])
def test_listed_pairs_past_the_grid_are_the_restatements(dims):
    t0 = time.perf_counter()
    g, x = graph("medium"), positions("medium", dims, "noisy")
    sa, sb = listed_pairs(g)
    assert sa.shape[0] == 600_000 > 2048 * 256
    ia, ib = sa.astype(np.int64), sb.astype(np.int64)
    pth = path_of_step(g)
    same = np.flatnonzero(pth[ia] == pth[ib])
    _, rel, ok = np_pair_values(g, x, dims, ia[same], ib[same])
    want = np.full(sa.shape[0], -1.0)
    want[same[ok]] = rel
    # the kinds of pairs the list is meant to hold
    assert (ia == ib).sum() >= 20000 and (pth[ia] != pth[ib]).sum() >= 30000 and (g.step_node[ia] == NO_NODE).sum() >= 20000
    assert (g.step_node[ib] == NO_NODE).sum() >= 20000 and (want[100000:140000] == -1.0).sum() >= 30000 and (ia > ib).sum() >= 50000
    assert (want[2048 * 256:] >= 0).sum() > 50000                         # counted pairs past the grid
    ctx = context(g, dims, x)
    stress, counted, got = ctx.stress_of_pairs(sa, sb)
    ctx.close()
    assert counted == int(ok.sum()) == int((got >= 0).sum())
    differ = np.flatnonzero(bits(got) != bits(want))
    assert differ.size == 0, (differ.size, differ[:5], got[differ[:5]], want[differ[:5]])
    total = 0.0
    for v in want[want >= 0].tolist():                                    # summed in list order
        total += v
    assert stress == np.sqrt(total / counted)
    table_row(f"K7b medium D={dims} 600000 listed", g, counted, t0)


# ---- K6, K7c --------------------------------------------------------------------------------------------------------------------
def test_sort_order_and_sort_quality_over_more_nodes_than_threads():
    t0 = time.perf_counter()
    g = graph("large")
    x = np.round(shuffled_start(g, 0, 2) / 40.0) * 40.0                  # multiples of 40 bp: many ties; far from sorted, so that
                                                                         # the squared errors add up to more than 2^53
    x[5:4000:7], x[6:4000:7] = -0.0, 0.0                                 # both zeros, in dense order between each other
    x[270000:270100:2], x[270001:270100:2] = 0.0, -0.0                   # ... also past the first 262 144 nodes
    assert np.unique(x).shape[0] < g.n_nodes // 4 and np.signbit(x[x == 0.0]).sum() > 500 and (~np.signbit(x[x == 0.0])).sum() > 500
    ctx = context(g, 0, x)
    order = ctx.sort_order()
    assert np.array_equal(order, np.argsort(x + 0.0, kind="stable").astype(np.uint64))
    q = ctx.sort_quality()
    assert ctx.sort_quality() == q
    ctx.close()
    want = np_sort_quality(g, order)
    for k in ("steps", "abs_err_sum", "genomic_sum"):
        assert q[k] == want[k], k
    ae, counted = sort_step_values(g, order)
    assert int(counted.sum()) == want["steps"] and int(ae.sum()) == want["abs_err_sum"]
    sq = ae.astype(np.float64) * ae.astype(np.float64)
    tree, plain = tree_sum(sq, counted, g.n_steps), float(sq[counted].sum())
    print("K7c sq_err_sum", repr(q["sq_err_sum"]), "tree", repr(tree), "numpy", repr(plain))
    assert plain > 2.0 ** 53                                              # the additions round: the order shows
    assert bits(q["sq_err_sum"]) == bits(tree)
    assert abs(q["sq_err_sum"] - plain) <= want["steps"] * U * plain
    table_row("K6+K7c large D=0", g, want["steps"], t0)


# ---- K7d ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noisy", "shuffled"])
@pytest.mark.parametrize("dims", [0, 2, 8])
def test_path_errors_over_more_than_64_tiles(dims, kind):
    t0 = time.perf_counter()
    g, x = graph("medium"), positions("medium", dims, kind)
    _, loads = path_counts_from_tiles(g, np.ones(g.n_steps))
    n1, n2, n3 = int((loads == 1).sum()), int((loads == 2).sum()), int((loads >= 3).sum())
    print("combine loads per path: one", n1, "two", n2, "three or more", n3, "none (inside one tile, or no steps)", int((loads == 0).sum()))
    assert n1 >= 5 and n2 >= 5 and n3 >= 1
    ctx = context(g, dims, x)
    pairs = 0
    for z in ZS["medium"]:
        k7a = ctx.pair_errors([z])
        for ratio in (10.0, 1.5):
            w = grouped(g, x, dims, z, ratio)["paths"]
            got = ctx.path_errors(z, ratio)
            for k in ("steps", "reverse_steps", "pairs", "stretched", "max_rel_sq"):
                bad = np.flatnonzero(got[k] != w[k])
                assert bad.size == 0, (k, z, ratio, bad[:5], got[k][bad[:5]], w[k][bad[:5]], loads[bad[:5]])
            for k in SUMS:
                assert np.all(np.abs(got[k] - w[k]) <= w["pairs"] * U * np.abs(w[k])), (k, z, ratio)
            assert int(got["pairs"].sum()) == int(k7a["pairs"][0])
            assert float(got["max_rel_sq"].max()) == float(k7a["max_rel_sq"][0])
            assert got.tobytes() == ctx.path_errors(z, ratio).tobytes()  # two calls: identical bytes
            if kind == "shuffled" and ratio == 10.0 and z == 1:
                assert 4 * int(got["stretched"].sum()) >= int(got["pairs"].sum())
        pairs += int(k7a["pairs"][0])
    if kind == "noisy":
        assert int(k7a["pairs"][0]) == k7a_wanted("medium", dims, ZS["medium"][-1])["pairs"]
    ctx.close()
    table_row(f"K7d medium D={dims} {kind} z={ZS['medium']} x 2 ratios", g, pairs, t0)


# ---- K7e ------------------------------------------------------------------------------------------------------------------------
def assert_listed(ctx, z, ratio, cap, w):
    """The first min(cap, total) entries exact, the total exact, the rest of the caller's buffer untouched."""
    total = w.shape[0]
    buf = np.zeros(cap + 3, dtype=hip.STRETCHED_PAIR_DTYPE)
    buf[:] = SENTINEL
    got, t = ctx.stretched_pairs(z, ratio, cap=cap, out=buf) if cap else ctx.stretched_pairs(z, ratio, cap=0)
    n = min(cap, total)
    assert t == total and got.shape[0] == n
    for k in hip.STRETCHED_PAIR_DTYPE.names:                              # field by field, the doubles as bits
        assert np.array_equal(got[k].view(np.uint64), w[k][:n].view(np.uint64)), (k, z, cap)
    assert np.all(buf[n:] == np.array(SENTINEL, dtype=hip.STRETCHED_PAIR_DTYPE))


@pytest.mark.parametrize("dims", [0, 2, 8])
def test_stretched_pairs_over_a_thousand_tiles(dims):
    t0 = time.perf_counter()
    g, x = graph("medium"), positions("medium", dims, "shuffled")
    ctx = context(g, dims, x)
    listed = 0
    for z in (1, 65):
        e = grouped(g, x, dims, z, 10.0)
        w, total = e["list"], e["list"].shape[0]
        print("medium shuffled dims", dims, "z", z, "stretched", total, "of", e["counted"])
        assert 4 * total >= e["counted"] > 400000                        # first: most pairs are stretched
        for cap in (total, total - 1, 1000, 0):
            assert_listed(ctx, z, 10.0, cap, w)
        listed += total
    ctx.close()
    table_row(f"K7e medium D={dims} shuffled z=[1, 65] x 4 caps", g, listed, t0)


# ---- K7e, K7f on `large` ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,z", [(0, 1), (0, 1000), (2, 1), (2, 1000)])
def test_node_errors_and_the_ends_of_the_stretched_list_on_large(dims, z):
    t0 = time.perf_counter()
    g, x = graph("large"), positions("large", dims, "shuffled")
    e = grouped(g, x, dims, z, 10.0)
    ctx = context(g, dims, x)
    got = ctx.node_errors(z, 10.0)
    for k in ("pairs", "stretched", "max_rel_sq"):
        bad = np.flatnonzero(got[k] != e["nodes"][k])
        assert bad.size == 0, (k, bad[:5], got[k][bad[:5]], e["nodes"][k][bad[:5]])
    assert int(got["pairs"][262144:].sum()) > 100000                     # nodes past the gather's 1024 x 256 threads
    assert got.tobytes() == ctx.node_errors(z, 10.0).tobytes()
    w, total = e["list"], e["list"].shape[0]
    assert 4 * total >= e["counted"] > 3_000_000
    assert_listed(ctx, z, 10.0, 1000, w)                                 # the first 1000
    full, t = ctx.stretched_pairs(z, 10.0, cap=total)
    assert t == total and full.shape[0] == total
    assert full[-1000:].tobytes() == w[-1000:].tobytes()                 # the last 1000
    assert ctx.stretched_pairs(z, 10.0, cap=0)[1] == total
    ctx.close()
    table_row(f"K7e+K7f large D={dims} shuffled z={z}", g, e["counted"], t0)


# ---- K7g ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2])
def test_a_batch_item_with_257_workgroups_behind_another_item(dims):
    """A batch is all sorts or all layouts of one dimension (gfs_batch_create refuses a mix): one batch per kind."""
    t0 = time.perf_counter()
    names = ["DRB1", "medium", "lil"]
    zs = ZS["medium"]
    cfg = hip.make_config(n_streams=64, flags=hip.F_BUNDLE(1))
    xs = [positions("medium", dims, "noisy") if n == "medium" else noisy_start(graph(n), dims, 31 + i) for i, n in enumerate(names)]
    ctxs = [context(graph(n), dims, x, cfg=cfg) for n, x in zip(names, xs)]
    assert quality_blocks_of(graph("DRB1").n_steps) == 18 and quality_blocks_of(graph("medium").n_steps) == 257
    b = hip.Batch(ctxs)
    rows = b.pair_errors(zs)
    assert rows.shape == (3, len(zs))
    for i, c in enumerate(ctxs):
        assert rows[i].tobytes() == c.pair_errors(zs).tobytes(), names[i]
    for row in rows[1]:                                                   # ... and therefore the tree
        assert_row_is_the_tree(ctxs[1], "medium", dims, row)
    assert b.pair_errors(zs).tobytes() == rows.tobytes()
    b.close()
    for c in ctxs:
        c.close()
    table_row(f"K7g [DRB1, medium, lil] D={dims} z={zs}", graph("medium"), rows["pairs"].sum(), t0)


# ---- a rank's shard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A-w3-anneal-f32-e1", "D-windows-d2-w3-anneal-f32"])
def test_readouts_of_a_shard_context_cover_the_shard_in_its_own_path_numbering(cid):
    """One rank's context by itself (the set-up of test_gpu_multi_merge.py's control): the shard's paths as a graph of their own
    over ALL nodes, the shared node layout as node_perm.  The figures are the restatement's on that subgraph: paths numbered
    as the shard numbers them, nodes by dense index of the whole graph, nodes the shard does not visit zero."""
    import multi_cases as MC
    t0 = time.perf_counter()
    case = MC.BY_ID[cid]
    g, plan, rank, dims = MC.graph(case.graph), MC.cluster(case).plan, 1, case.dims
    mine = plan.paths_of(rank)
    sub = subgraph(g, mine)
    assert 0 < len(mine) < g.n_paths and sub.n_nodes == g.n_nodes and sub.n_steps < g.n_steps
    x = noisy_start(g, dims, 11)
    ctx = context(sub, dims, x, node_perm=plan.perm)
    assert np.array_equal(ctx.node_layout(), plan.perm)
    pairs = 0
    for z in (1, 65):
        row = ctx.pair_errors([z])[0]
        want = np_pair_errors(sub, x, dims, z)
        assert int(row["pairs"]) == want["pairs"] > 0 and float(row["max_rel_sq"]) == want["max_rel_sq"]
        v = step_values(sub, x, dims, z)
        for k in SUMS:
            assert bits(row[k]) == bits(tree_sum(v[STEP_VALUE_OF[k]], v["counted"], sub.n_steps)), (k, z)
            assert abs(float(row[k]) - want[k]) <= want["pairs"] * U * abs(want[k]), (k, z)
        e = grouped(sub, x, dims, z, 1.5)
        got = ctx.path_errors(z, 1.5)
        assert got.shape[0] == len(mine)
        for k in ("steps", "reverse_steps", "pairs", "stretched", "max_rel_sq"):
            assert np.array_equal(got[k], e["paths"][k]), (k, z)
        for k in SUMS:
            assert np.all(np.abs(got[k] - e["paths"][k]) <= e["paths"]["pairs"] * U * np.abs(e["paths"][k])), (k, z)
        assert np.array_equal(got["steps"].astype(np.int64), g.path_step_counts()[mine])
        nodes = ctx.node_errors(z, 1.5)
        for k in ("pairs", "stretched", "max_rel_sq"):
            assert np.array_equal(nodes[k], e["nodes"][k]), (k, z)
        visited = np.zeros(g.n_nodes, dtype=bool)
        visited[sub.step_node[sub.step_node != NO_NODE]] = True
        assert (~visited).sum() > 0 and not nodes["pairs"][~visited].any() and int(e["paths"]["stretched"].sum()) > 0
        pairs += want["pairs"]
    ctx.close()
    table_row(f"shard of rank 1, {cid} z=[1, 65]", sub, pairs, t0)
