"""Batches of layouts, fed and read as a batch (K4c / K6c, batch_quality_kernels.hip): gfs_batch_upload_coords and gfs_batch_coords
move every item's coordinates as one packed array and give, per item, the bits of gfs_ctx_upload_positions and
gfs_ctx_download_positions; and the whole path — upload, one persistent launch, read-out — up to the Python one-call form and the
CLI.  Every expectation is the item's own context calls, the oracle, or the single run: the kernel under test is never compared
with itself."""
import functools
import os
import re
import subprocess
import time

import numpy as np
import pytest

from util import O, G, P, load, oracle_graph, oracle_params, gaussian_init
from gfasort_amd import build, hip
from gfasort_amd import sgd as S

pytestmark = pytest.mark.gpu

FIXTURES = ("simple.gfa", "lil.gfa", "DRB1-3123.gfa")
E_ARG, E_UNSUPPORTED = -1, -5
SEAM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257)            # words per item 4n (D = 2), 6n (D = 3): wave and workgroup edges


def _chain(n, seed):
    """One path over n nodes of lengths 1..16, whose S lines come in another order than the path visits them."""
    rng = np.random.default_rng(seed)
    s_order = rng.permutation(n) + 1
    if n > 1 and np.array_equal(s_order, np.arange(1, n + 1)):
        s_order = s_order[::-1]
    lines = ["S\t%d\t%s" % (nid, "A" * (1 + (nid - 1) % 16)) for nid in s_order]
    lines.append("P\tp\t" + ",".join("%d+" % nid for nid in range(1, n + 1)) + "\t*")
    return G.parse_gfa("\n".join(lines) + "\n")


def _layout_params(g, dims, iter_max=5, seed=None, min_term_updates=None):
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = iter_max
    if seed is not None:
        p.seed = seed
    if min_term_updates is not None:
        p.min_term_updates = min_term_updates
    return p


def _crafted(n, seed):
    """Doubles with what a copy can get wrong: both zeros, infinities, a denormal, NaNs with payloads."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1000.0, n)
    special = np.array([-0.0, np.inf, -np.inf, 5e-324, 0.0], dtype=np.float64)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000123, 0x7FF0000000000001], dtype=np.uint64).view(np.float64)
    picks = rng.permutation(n)
    for k, v in zip(picks, np.concatenate([nans[:1], special, nans[1:]])):   # (as many as the item has room for: 4 words at least)
        x[k] = v
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", params=[2, 3])
def seams(request):
    """The seams batch of one dimension, built once: (D, contexts, batch)."""
    D = request.param
    graphs = [_chain(n, 100 + n) for n in SEAM_SIZES[:4]]
    graphs += [load("lil.gfa"), G.parse_gfa("S\t1\tAC\nS\t2\tG\nP\ta\t1+\t*\nP\tb\t2+\t*\n"), load("simple.gfa")]   # idle in the middle
    graphs += [_chain(n, 100 + n) for n in SEAM_SIZES[4:]]
    ctxs = []
    for i, g in enumerate(graphs):
        ctx = hip.Context(g)
        rc = ctx.setup_nd(_layout_params(g, D, 2), hip.make_config(n_streams=1))
        assert (rc == hip.NOTHING_TO_DO) == (int(np.diff(g.path_first_step.astype(np.int64)).max()) < 2), i
        assert (rc == hip.NOTHING_TO_DO) == (i in (0, 5))              # the one-node chain has nothing to do either
        assert ctx.positions_len() == g.n_nodes * 2 * D
        ctxs.append(ctx)
    assert any(not np.array_equal(c.node_layout(), np.arange(c.graph.n_nodes)) for c in ctxs)   # the planes are scattered into
    b = hip.Batch(ctxs)
    yield D, ctxs, b
    b.close()
    for c in ctxs:
        c.close()


def test_upload_at_the_seams(seams):
    D, ctxs, b = seams
    sizes = [c.graph.n_nodes for c in ctxs]
    assert set(SEAM_SIZES) <= set(sizes)
    off = b.coords_offsets()
    assert np.array_equal(off, (np.concatenate([[0], np.cumsum(sizes)]) * 2 * D).astype(np.uint64))
    for c in ctxs:
        c.upload(np.full(c.positions_len(), -7.0))                     # (whatever was there is overwritten)
    xs = [_crafted(n * 2 * D, 9000 + 10 * D + i) for i, n in enumerate(sizes)]
    assert any(np.isnan(x).any() for x in xs) and any((_bits(x) == np.uint64(1) << np.uint64(63)).any() for x in xs)
    b.upload_coords(xs)
    for i, c in enumerate(ctxs):
        assert np.array_equal(_bits(c.download()), _bits(xs[i])), (D, i, sizes[i])
    packed = np.concatenate(xs[::-1])                                  # the packed form: other values everywhere
    b.upload_coords(packed)
    for i, c in enumerate(ctxs):
        assert np.array_equal(_bits(c.download()), _bits(packed[int(off[i]):int(off[i + 1])])), (D, i)


def test_read_out_at_the_seams(seams):
    D, ctxs, b = seams
    xs = [_crafted(c.positions_len(), 500 + 10 * D + i) for i, c in enumerate(ctxs)]
    for c, x in zip(ctxs, xs):
        c.upload(x)                                                    # per item, through the context
    coords, ms = b.coords()
    print("D", D, "read-out of", len(ctxs), "items: kernel_ms", ms)
    assert ms > 0.0 and len(coords) == len(ctxs)
    for i, c in enumerate(ctxs):
        assert coords[i].shape == (c.positions_len(),)
        assert np.array_equal(_bits(coords[i]), _bits(c.download())) and np.array_equal(_bits(coords[i]), _bits(xs[i])), (D, i)
    again, _ = b.coords()
    assert all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(again, coords))


def test_total_is_exact(seams):
    D, ctxs, b = seams
    total = sum(c.positions_len() for c in ctxs)
    x = np.zeros(total + 2)
    L = hip.lib()
    for wrong in (total - 1, total + 1, 0, total // (2 * D)):
        assert L.gfs_batch_upload_coords(b._h, x.ctypes.data, wrong, None) == E_ARG
        assert L.gfs_batch_coords(b._h, x.ctypes.data, wrong, None, None) == E_ARG
    assert L.gfs_batch_upload_coords(b._h, None, total, None) == E_ARG
    assert L.gfs_batch_coords(b._h, None, total, None, None) == E_ARG
    guard = np.full(total + 2, 123.25)
    assert L.gfs_batch_coords(b._h, guard.ctypes.data, total, None, None) == 0
    assert guard[total] == 123.25 and guard[total + 1] == 123.25       # nothing beyond the last item


def test_wrong_kind_is_refused_by_name():
    g = load("simple.gfa")
    p1 = P.YgsParams.from_graph(g, 0, 1).path_sgd
    sorts = []
    for seed in (1, 2):
        c = hip.Context(g)
        p1.seed = seed
        assert c.setup_1d(p1, hip.make_config(n_streams=1)) == hip.OK
        sorts.append(c)
    sb = hip.Batch(sorts)
    x = np.zeros(4 * g.n_nodes * 2)
    with pytest.raises(hip.GfsError) as ei:
        sb.upload_coords(x)
    assert ei.value.code == E_UNSUPPORTED and "gfs_batch_results" in str(ei.value)
    with pytest.raises(hip.GfsError) as ei:
        sb.coords()
    assert ei.value.code == E_UNSUPPORTED and "gfs_batch_results" in str(ei.value)
    sb.close()
    lay = []
    for seed in (1, 2):
        c = hip.Context(g)
        assert c.setup_nd(_layout_params(g, 2, 2, seed), hip.make_config(n_streams=1)) == hip.OK
        lay.append(c)
    lb = hip.Batch(lay)
    for call in (lb.init_positions, lb.results):
        with pytest.raises(hip.GfsError) as ei:
            call()
        assert ei.value.code == E_UNSUPPORTED and "gfs_batch_upload_coords" in str(ei.value) and "gfs_batch_coords" in str(ei.value)
    lb.close()


@functools.lru_cache(maxsize=None)
def _oracle_layout(name):
    """(start, final coordinates, term_updates, attempts) of the oracle's single stream at D = 2; computed once, never written to."""
    g = load(name)
    p = _layout_params(g, 2, 5, min_term_updates=12000 if name.startswith("DRB1") else None)
    c0 = gaussian_init(g, 2, 7)
    c = c0.copy()
    rc, st, _ = O.sgd_nd(oracle_graph(g), oracle_params(p), c, n_streams=1)
    assert rc == 0
    c0.setflags(write=False)
    c.setflags(write=False)
    return c0, c, st.term_updates, st.attempts


def _fixture_ctx(name):
    g = load(name)
    ctx = hip.Context(g)
    assert ctx.setup_nd(_layout_params(g, 2, 5, min_term_updates=12000 if name.startswith("DRB1") else None), hip.make_config(n_streams=1)) == hip.OK
    return ctx


def test_upload_run_and_read_out_equal_the_oracle():
    ctxs = [_fixture_ctx(name) for name in FIXTURES]
    b = hip.Batch(ctxs)
    b.upload_coords([_oracle_layout(name)[0] for name in FIXTURES])
    b.run()
    assert b.stats().launches == 1 and b.stats().items_run == 3
    coords, _ = b.coords()
    for i, name in enumerate(FIXTURES):
        _, c_ref, updates, attempts = _oracle_layout(name)
        st = ctxs[i].stats()
        assert (st.term_updates, st.attempts, st.bundle) == (updates, attempts, 1), name
        assert np.array_equal(_bits(coords[i]), _bits(c_ref)), name
    b.close()


def test_many_items_equal_their_solo_runs():
    """48 items of one stream each, one launch: every item is what the same kind of context gives with its own upload, run
    and download."""
    graphs = [load("simple.gfa"), load("lil.gfa")]
    ctxs, starts, solo = [], [], []
    for i in range(48):
        g = graphs[i % 2]
        p = _layout_params(g, 2, 5, seed=9399220 + i)
        c0 = gaussian_init(g, 2, 50 + i)
        own = hip.Context(g)
        assert own.setup_nd(p, hip.make_config(n_streams=1)) == hip.OK
        own.upload(c0)
        own.run()
        solo.append((own.download(), own.stats().term_updates, own.stats().attempts))
        own.close()
        ctx = hip.Context(g)
        assert ctx.setup_nd(p, hip.make_config(n_streams=1)) == hip.OK
        ctxs.append(ctx)
        starts.append(c0)
    b = hip.Batch(ctxs)
    b.upload_coords(starts)
    b.run()
    assert (b.stats().launches, b.stats().items_run, b.stats().blocks) == (1, 48, 48)
    coords, _ = b.coords()
    for i, (x, updates, attempts) in enumerate(solo):
        st = ctxs[i].stats()
        assert np.array_equal(_bits(coords[i]), _bits(x)), i
        assert (st.term_updates, st.attempts) == (updates, attempts), i
    assert len({c.tobytes() for c in coords}) == 48                    # (48 different runs)
    b.close()


def test_python_layout_batch_equals_single_calls():
    graphs = [load(name) for name in FIXTURES]
    params = [_layout_params(g, 2, 5, min_term_updates=12000 if name.startswith("DRB1") else None) for g, name in zip(graphs, FIXTURES)]
    cfg = hip.make_config(n_streams=1)
    out, bs = S.path_linear_sgd_layout_batch(graphs, params, cfg=cfg)
    assert list(bs) == [2] and bs[2].launches == 1 and bs[2].items_run == 3
    for res, g, p in zip(out, graphs, params):
        lay, st = S.path_linear_sgd_layout(g, p, cfg=cfg, return_stats=True)
        assert res["batched"] and res["layout"].dimensions == 2 and res["layout"].num_nodes == g.n_nodes
        assert np.array_equal(_bits(res["layout"].coords), _bits(lay.coords)), g.n_nodes
        assert (res["stats"].term_updates, res["stats"].attempts) == (st.term_updates, st.attempts)
    # a start of the caller's, and a graph that cannot be in the batch (4 dimensions) in the same call
    inits = [_oracle_layout(FIXTURES[0])[0], None, None]
    params[1] = _layout_params(graphs[1], 4, 5)
    out, bs = S.path_linear_sgd_layout_batch(graphs, params, inits=inits, cfg=cfg)
    assert [r["batched"] for r in out] == [True, False, True] and bs[2].items_run == 2
    assert np.array_equal(_bits(out[0]["layout"].coords), _bits(_oracle_layout(FIXTURES[0])[1]))
    lay = S.path_linear_sgd_layout(graphs[1], params[1], cfg=cfg)
    assert out[1]["layout"].dimensions == 4 and np.array_equal(_bits(out[1]["layout"].coords), _bits(lay.coords))


PROFILE = re.compile(r"^\[gfasort\] stress profile: .*$", re.M)


@pytest.mark.parametrize("pipeline", ["L", "Y"])
def test_cli_batch_writes_what_single_runs_write(tmp_path, pipeline):
    """--batch LIST against one invocation per graph: the GFA files and, for -p L, the layout files as bytes; with
    --stress-profile the profile lines on stderr, graph by graph."""
    build.build_host()
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    flags = ["-p", pipeline, "--streams", "1", "-v", "1", "--stress-profile"] + (["--layout-iter", "1"] if pipeline == "L" else ["--iter-max", "10"])
    lines, solo_profile = [], []
    for name in FIXTURES:
        src = os.path.join(data, name)
        cmd = [build.CLI, "-i", src, "-o", str(tmp_path / ("solo_" + name))] + flags
        if pipeline == "L":
            cmd += ["--layout-out", str(tmp_path / ("solo_" + name + ".tsv"))]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows = PROFILE.findall(r.stderr)
        assert rows
        solo_profile += rows
        lines.append("\t".join([src, str(tmp_path / ("batch_" + name))] + ([str(tmp_path / ("batch_" + name + ".tsv"))] if pipeline == "L" else [])) + "\n")
    (tmp_path / "list.tsv").write_text("".join(lines))
    r = subprocess.run([build.CLI, "--batch", str(tmp_path / "list.tsv")] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "3 graphs in 1 launch" in r.stderr and r.stderr.count("in the batch") == 3, r.stderr
    for name in FIXTURES:
        assert (tmp_path / ("batch_" + name)).read_bytes() == (tmp_path / ("solo_" + name)).read_bytes(), name
        if pipeline == "L":
            tsv = (tmp_path / ("batch_" + name + ".tsv")).read_bytes()
            assert tsv == (tmp_path / ("solo_" + name + ".tsv")).read_bytes() and tsv.count(b"\n") > 1, name
    assert PROFILE.findall(r.stderr) == solo_profile


def test_one_call_is_faster_than_the_per_item_loop():
    """64 DRB1 items at D = 2 after a short run: batched upload + read-out + pair errors at the default ladder against the loop of
    context calls on the same contexts, host wall time, the median of 5 after an untimed call of each.  A condition, not a tuned
    number: the loop makes 64 x (2 allocations + 2 launches of 2048 workgroups + 2 pageable copies + 3 synchronises + K7a's pair)."""
    from gfasort_amd import quality as Q
    g = load("DRB1-3123.gfa")
    zs = Q.step_distance_ladder(int(np.diff(g.path_first_step.astype(np.int64)).max()))
    ctxs = []
    for i in range(64):
        ctx = hip.Context(g)
        assert ctx.setup_nd(_layout_params(g, 2, 1, seed=9399220 + 1000 * i)) == hip.OK
        ctxs.append(ctx)
    starts = [gaussian_init(g, 2, 7 + i) for i in range(4)]
    starts = [starts[i % 4] for i in range(64)]
    b = hip.Batch(ctxs)
    b.upload_coords(starts)
    b.run()

    def batched():
        b.upload_coords(starts)
        return b.coords(), b.pair_errors(zs, return_ms=True)

    def loop():
        for c, x in zip(ctxs, starts):
            c.upload(x)
        return [c.download() for c in ctxs], [c.pair_errors(zs) for c in ctxs]

    def median(f):
        f()                                                            # untimed: code objects, scratch
        times, last = [], None
        for _ in range(5):
            t0 = time.perf_counter()
            last = f()
            times.append(time.perf_counter() - t0)
        return float(np.median(times)), last
    t_batch, ((coords, ms_coords), (rows, ms_pairs)) = median(batched)
    t_loop, (xs, loop_rows) = median(loop)
    print("64 DRB1 items, D = 2, %d step distances: batched %.3f ms (kernel_ms: coordinates %.3f, pair errors %.3f), per-item loop %.3f ms"
          % (len(zs), t_batch * 1e3, ms_coords, ms_pairs, t_loop * 1e3))
    for i in range(64):
        assert np.array_equal(_bits(coords[i]), _bits(xs[i])) and rows[i].tobytes() == loop_rows[i].tobytes(), i
    assert t_batch < t_loop, (t_batch, t_loop)
    b.close()


def test_cli_batch_layout_runs_every_refused_graph_alone(tmp_path):
    """-p L with the flags above plus --hip-flags 4 (GFS_F_NO_FUSE: no fused launch, so no graph may be in a batch): the batch is
    refused item after item until nothing is left, every graph runs alone after that, and writes what its single run writes."""
    from util import cli_solo_and_batch
    build.build_host()
    flags = ["-p", "L", "--streams", "1", "-v", "1", "--stress-profile", "--layout-iter", "1", "--hip-flags", "4"]
    solo, r = cli_solo_and_batch(build.CLI, tmp_path, FIXTURES, flags, layouts=True)
    assert all(s.returncode == 0 for s in solo), [s.stderr for s in solo]
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("runs alone") == len(FIXTURES) and "in the batch" not in r.stderr, r.stderr
    for name in FIXTURES:
        assert (tmp_path / ("batch_" + name)).read_bytes() == (tmp_path / ("solo_" + name)).read_bytes(), name
        tsv = (tmp_path / ("batch_" + name + ".tsv")).read_bytes()
        assert tsv == (tmp_path / ("solo_" + name + ".tsv")).read_bytes() and tsv.count(b"\n") > 1, name


def test_python_layout_batch_runs_a_refused_graph_alone():
    """The layout twin of test_python_batch_sort_runs_a_refused_graph_alone.  One launch may hold one workgroup here: lil at 1000
    streams (more than the 256 of one workgroup) cannot be in the batch and runs alone, after the batch; the other two still run
    as a batch, each with the bits of its own single call at one stream."""
    graphs = [load(name) for name in FIXTURES]
    params = [_layout_params(g, 2, 5, min_term_updates=12000 if name.startswith("DRB1") else None) for g, name in zip(graphs, FIXTURES)]
    one, wide = hip.make_config(n_streams=1), hip.make_config(n_streams=1000)
    ctx = hip.Context(graphs[1])
    assert ctx.setup_nd(params[1], wide) == hip.OK
    assert ctx.stats().n_streams > 256 and ctx.stats().bundle == 1          # (the policy does not cap what was asked for)
    ctx.close()
    out, bs = S.path_linear_sgd_layout_batch(graphs, params, cfg=[one, wide, one], max_blocks_per_launch=1)
    assert [r["batched"] for r in out] == [True, False, True]
    assert list(bs) == [2] and (bs[2].items, bs[2].items_run) == (2, 2)
    for i in (0, 2):
        lay = S.path_linear_sgd_layout(graphs[i], params[i], cfg=one)
        assert np.array_equal(_bits(out[i]["layout"].coords), _bits(lay.coords)), i
    assert out[1]["stats"].n_streams == 1000 and np.isfinite(out[1]["layout"].coords).all()
    assert out[1]["layout"].num_nodes == graphs[1].n_nodes
