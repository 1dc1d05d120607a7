"""Batches (gfs_batch, K1f / K2f): many set-up contexts in one persistent launch.  An item of a batch is exactly what a launch of
that context alone is: one stream per item is the oracle's single stream bit for bit, whatever runs beside it; at full width every
item applies its exact number of updates and reaches the quality of a solo run; and the batch takes less kernel time than its
items one after the other."""
import functools
import os
import subprocess

import numpy as np
import pytest

from util import O, G, P, load, oracle_graph, oracle_params, gaussian_init
from gfasort_amd import build, hip

pytestmark = pytest.mark.gpu

FIXTURES = (("simple.gfa", 100), ("lil.gfa", 100), ("DRB1-3123.gfa", 10))
E_UNSUPPORTED = -5


def _ygs(g, iter_max, seed=None):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    if seed is not None:
        p.seed = seed
    return p


@functools.lru_cache(maxsize=None)
def _oracle_one_stream(name, iter_max, seed=9399220):
    """(positions, term_updates, attempts) of the oracle's single stream; computed once, never written to."""
    g = load(name)
    p = _ygs(g, iter_max, seed)
    og = oracle_graph(g)
    x = O.init_positions(og)
    rc, st, _ = O.sgd_1d(og, oracle_params(p), x, n_streams=1)
    assert rc == 0
    x.setflags(write=False)
    return x, st.term_updates, st.attempts


def _ctx_1d(g, p, **cfg):
    ctx = hip.Context(g)
    rc = ctx.setup_1d(p, hip.make_config(**cfg))
    if rc == hip.OK:
        ctx.init_positions()
    return ctx


def _fixture_batch(flags=(0, 0, 0)):
    ctxs = []
    for (name, iter_max), f in zip(FIXTURES, flags):
        g = load(name)
        ctxs.append(_ctx_1d(g, _ygs(g, iter_max), n_streams=1, flags=f))
    return ctxs


def _check_fixture_items(ctxs):
    for ctx, (name, iter_max) in zip(ctxs, FIXTURES):
        x_ref, updates, attempts = _oracle_one_stream(name, iter_max)
        st = ctx.stats()
        print(name, "updates", st.term_updates, updates, "attempts", st.attempts, attempts)
        assert np.array_equal(ctx.download().view(np.uint64), x_ref.view(np.uint64)), name
        assert (st.term_updates, st.attempts) == (updates, attempts), name
        assert st.term_updates == (iter_max + 1) * ctx.params.min_term_updates
        assert st.iterations == iter_max + 1 and st.launches == 1 and st.kernel_ms == 0.0


@pytest.mark.parametrize("flags,launches", [((0, 0, 0), 1), ((hip.F_NO_LDS_TABLES,) * 3, 1), ((0, hip.F_NO_LDS_TABLES, 0), 2)])
def test_one_launch_is_bit_exact(flags, launches):
    ctxs = _fixture_batch(flags)
    b = hip.Batch(ctxs)
    assert b.run() == hip.OK
    bs = b.stats()
    assert (bs.launches, bs.items, bs.items_run, bs.blocks) == (launches, 3, 3, 3)
    _check_fixture_items(ctxs)
    assert bs.term_updates == sum(_oracle_one_stream(n, k)[1] for n, k in FIXTURES)
    assert bs.attempts == sum(_oracle_one_stream(n, k)[2] for n, k in FIXTURES)
    assert bs.kernel_ms > 0.0
    b.close()


def test_split_launches():
    ctxs = _fixture_batch()
    b = hip.Batch(ctxs, max_blocks_per_launch=1)
    b.run()
    assert b.stats().launches == 3
    _check_fixture_items(ctxs)
    b.close()
    g = load("lil.gfa")
    wide = _ctx_1d(g, _ygs(g, 100), n_streams=1000)                    # 4 workgroups of 256
    with pytest.raises(hip.GfsError) as ei:
        hip.Batch([ctxs[0], wide], max_blocks_per_launch=1)
    assert ei.value.code == E_UNSUPPORTED and "item 1" in str(ei.value)


@pytest.mark.parametrize("dims", [2, 3])
def test_layout_items_equal_oracle(dims):
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    ctxs, refs = [], []
    for seed in (None, 4242):
        p = P.LayoutSGDParams.from_graph(g, dims, 1)
        p.iter_max = 5                                                 # crosses into the cooling half
        p.min_term_updates = 12000
        if seed is not None:
            p.seed = seed
        c0 = gaussian_init(g, dims, 7)
        c_ref = c0.copy()
        rc, st, _ = O.sgd_nd(og, oracle_params(p), c_ref, n_streams=1)
        assert rc == 0
        refs.append((c_ref, st))
        ctx = hip.Context(g)
        assert ctx.setup_nd(p, hip.make_config(n_streams=1)) == hip.OK
        ctx.upload(c0)
        ctxs.append(ctx)
    assert not np.array_equal(refs[0][0], refs[1][0])
    b = hip.Batch(ctxs)
    b.run()
    assert b.stats().launches == 1
    for ctx, (c_ref, st) in zip(ctxs, refs):
        hst = ctx.stats()
        assert (hst.term_updates, hst.attempts) == (st.term_updates, st.attempts) and hst.bundle == 1
        assert np.array_equal(ctx.download().view(np.uint64), c_ref.view(np.uint64))
    b.close()


def test_kinds_do_not_mix():
    g = load("simple.gfa")
    one = _ctx_1d(g, _ygs(g, 10), n_streams=1)
    lay = {}
    for dims in (2, 3):
        lay[dims] = hip.Context(g)
        assert lay[dims].setup_nd(P.LayoutSGDParams.from_graph(g, dims, 1), hip.make_config(n_streams=1)) == hip.OK
    for pair in ((one, lay[2]), (lay[2], lay[3])):
        with pytest.raises(hip.GfsError) as ei:
            hip.Batch(list(pair))
        assert ei.value.code == E_UNSUPPORTED and "item 1" in str(ei.value)
    with pytest.raises(hip.GfsError) as ei:
        hip.Batch([one, one])
    assert ei.value.code == -1 and "item 1" in str(ei.value)
    unfused = _ctx_1d(g, _ygs(g, 10), n_streams=1, flags=hip.F_NO_FUSE)
    with pytest.raises(hip.GfsError) as ei:
        hip.Batch([one, unfused])
    assert ei.value.code == E_UNSUPPORTED and "item 1" in str(ei.value)
    fresh = hip.Context(g)                                             # never set up
    with pytest.raises(hip.GfsError) as ei:
        hip.Batch([one, fresh])
    assert ei.value.code == -4 and "item 1" in str(ei.value)


def test_isolation_at_full_width():
    drb1, lil = load("DRB1-3123.gfa"), load("lil.gfa")
    x_ref, updates, attempts = _oracle_one_stream("DRB1-3123.gfa", 10)
    one = _ctx_1d(drb1, _ygs(drb1, 10), n_streams=1)
    full = _ctx_1d(drb1, _ygs(drb1, 10, seed=77))                      # default stream count: 5 workgroups
    ragged = _ctx_1d(lil, _ygs(lil, 100), n_streams=1000)              # 15 full waves and one of 40 lanes, 4 workgroups
    bystander = _ctx_1d(drb1, _ygs(drb1, 10, seed=5))                  # set up, initialised, not in the batch
    x_by = bystander.download()
    idle_g = G.parse_gfa("S\t1\tAC\nS\t2\tG\nP\ta\t1+\t*\nP\tb\t2+\t*\n")   # every path has one step
    idle = hip.Context(idle_g)
    assert idle.setup_1d(_ygs(idle_g, 10)) == hip.NOTHING_TO_DO
    x_idle = idle.download()
    b = hip.Batch([one, full, idle, ragged])
    b.run()
    bs = b.stats()
    assert (bs.items, bs.items_run, bs.launches) == (4, 3, 1)
    assert full.stats().n_streams > 256 and bs.blocks == 1 + (full.stats().n_streams + 255) // 256 + 4
    st = one.stats()
    assert np.array_equal(one.download().view(np.uint64), x_ref.view(np.uint64))
    assert (st.term_updates, st.attempts) == (updates, attempts)
    assert full.stats().term_updates == 11 * full.params.min_term_updates
    assert ragged.stats().term_updates == 101 * ragged.params.min_term_updates and ragged.stats().n_streams == 1000
    assert np.array_equal(bystander.download().view(np.uint64), x_by.view(np.uint64)) and bystander.stats().iterations == 0
    assert np.array_equal(idle.download().view(np.uint64), x_idle.view(np.uint64)) and idle.stats().iterations == 0
    assert not np.array_equal(full.download(), x_by)                   # (the full-width item did move)
    b.close()


def test_many_items_equal_their_solo_runs():
    graphs = [load("simple.gfa"), load("lil.gfa")]
    ctxs, solo = [], []
    for i in range(48):
        g = graphs[i % 2]
        p = _ygs(g, 100, seed=9399220 + i)
        rc, x, st = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1))
        assert rc == 0
        solo.append((x, st.term_updates, st.attempts))
        ctxs.append(_ctx_1d(g, p, n_streams=1))
    b = hip.Batch(ctxs)
    b.run()
    assert (b.stats().launches, b.stats().items_run, b.stats().blocks) == (1, 48, 48)
    for i, (ctx, (x, updates, attempts)) in enumerate(zip(ctxs, solo)):
        st = ctx.stats()
        assert np.array_equal(ctx.download().view(np.uint64), x.view(np.uint64)), i
        assert (st.term_updates, st.attempts) == (updates, attempts), i
    assert len({s[0].tobytes() for s in solo}) == 48                   # (48 different runs)
    b.close()


def test_running_twice_continues_the_streams():
    """Two runs of a batch are two gfs_ctx_run calls of every item: the streams go on where they stopped."""
    g = load("lil.gfa")
    p = _ygs(g, 20)
    alone = _ctx_1d(g, p, n_streams=1)
    alone.run()
    alone.run()
    item = _ctx_1d(g, p, n_streams=1)
    b = hip.Batch([item])
    b.run()
    b.run()
    assert np.array_equal(item.download().view(np.uint64), alone.download().view(np.uint64))
    assert item.stats().iterations == 42 and item.stats().launches == 2 and b.stats().launches == 2
    assert np.array_equal(item.sort_order(), alone.sort_order())
    b.close()


def test_quality_and_time_at_full_width():
    """DRB1 at the CLI's -p Y defaults, 8 items in one batch: the sampler is K1d's, so the bound on the final stress is that of
    test_reference_streams_fused_at_full_width_on_drb1 (means over seeds, max < 1.08 * min); and the batch must take less kernel
    time than its 8 items one after the other — the condition that batching does anything at all.  (The ratio itself is what
    scripts/batch_probe.py records.)"""
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    ctxs = [_ctx_1d(g, _ygs(g, 100, seed=9399220 + 1000 * i)) for i in range(8)]
    b = hip.Batch(ctxs)
    b.run()
    bs = b.stats()
    assert bs.launches == 1 and bs.term_updates == 8 * 101 * ctxs[0].params.min_term_updates
    s_batch = float(np.mean([O.stress_1d(og, c.download(), 200000) for c in ctxs]))
    solo_stress, solo_ms = [], 0.0
    for i in range(8):
        rc, x, st = hip.path_linear_sgd_raw(g, _ygs(g, 100, seed=9399220 + 1000 * i))
        assert rc == 0 and st.bundle == 1 and st.launches == 1
        solo_ms += st.kernel_ms
        if i < 3:
            solo_stress.append(O.stress_1d(og, x, 200000))
    s_solo = float(np.mean(solo_stress))
    x_ref = O.init_positions(og)
    O.sgd_1d(og, oracle_params(_ygs(g, 100)), x_ref, n_streams=64)
    s_ref = O.stress_1d(og, x_ref, 200000)
    print("stress: batch", s_batch, "solo", s_solo, "oracle", s_ref, "| kernel ms: batch", bs.kernel_ms, "sum of 8 solo", solo_ms)
    assert max(s_batch, s_solo, s_ref) < 1.08 * min(s_batch, s_solo, s_ref), (s_batch, s_solo, s_ref)
    assert bs.kernel_ms < solo_ms, (bs.kernel_ms, solo_ms)
    b.close()


def test_python_batch_sort_returns_per_graph_results():
    from gfasort_amd import sgd as S
    graphs = [load(name) for name, _ in FIXTURES]
    params = [_ygs(g, k) for g, (_, k) in zip(graphs, FIXTURES)]
    out, bs = S.path_sgd_sort_batch(graphs, params, cfg=hip.make_config(n_streams=1))
    assert bs.launches == 1 and bs.items_run == 3
    for res, (name, iter_max) in zip(out, FIXTURES):
        x_ref = _oracle_one_stream(name, iter_max)[0]
        assert res["batched"] and np.array_equal(res["positions"].view(np.uint64), x_ref.view(np.uint64))
        assert np.array_equal(res["order"], hip.sort_order(x_ref))


def test_python_batch_sort_runs_a_refused_graph_alone():
    """One launch may hold one workgroup here: lil at 1000 streams (4 workgroups) cannot be in the batch and runs alone; the other
    two still run as a batch (two launches of one workgroup), with the oracle's bits."""
    from gfasort_amd import sgd as S
    graphs = [load(name) for name, _ in FIXTURES]
    params = [_ygs(g, k) for g, (_, k) in zip(graphs, FIXTURES)]
    cfgs = [hip.make_config(n_streams=1), hip.make_config(n_streams=1000), hip.make_config(n_streams=1)]
    out, bs = S.path_sgd_sort_batch(graphs, params, cfg=cfgs, max_blocks_per_launch=1)
    assert [r["batched"] for r in out] == [True, False, True]
    assert (bs.items, bs.items_run, bs.launches) == (2, 2, 2)
    for i in (0, 2):
        x_ref = _oracle_one_stream(*FIXTURES[i])[0]
        assert np.array_equal(out[i]["positions"].view(np.uint64), x_ref.view(np.uint64))
    alone = out[1]["stats"]
    assert alone.n_streams == 1000 and alone.term_updates == 101 * params[1].min_term_updates and alone.kernel_ms > 0.0


def test_run_refuses_a_context_set_up_again():
    """The launches are cut at create.  A borrowed context that is set up again with another shape is an error of state at
    run(), and nothing is launched: the other item stays where it was."""
    g = load("lil.gfa")
    a, b_ = _ctx_1d(g, _ygs(g, 20), n_streams=1), _ctx_1d(g, _ygs(g, 20), n_streams=1)
    batch = hip.Batch([a, b_])
    x_a = a.download()
    assert b_.setup_1d(_ygs(g, 20), hip.make_config(n_streams=1000)) == hip.OK      # 4 workgroups where 1 was planned
    with pytest.raises(hip.GfsError) as ei:
        batch.run()
    assert ei.value.code == -4 and "item 1" in str(ei.value)
    assert np.array_equal(a.download().view(np.uint64), x_a.view(np.uint64)) and a.stats().iterations == 0
    assert b_.setup_1d(_ygs(g, 30), hip.make_config(n_streams=1)) == hip.OK         # another schedule length
    with pytest.raises(hip.GfsError) as ei:
        batch.run()
    assert ei.value.code == -4 and "item 1" in str(ei.value)
    batch.close()


def test_cli_batch_writes_what_single_runs_write(tmp_path):
    build.build_host()
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    flags = ["-p", "Y", "--streams", "1", "--iter-max", "10", "-v", "1"]
    lines = []
    for name, _ in FIXTURES:
        src = os.path.join(data, name)
        r = subprocess.run([build.CLI, "-i", src, "-o", str(tmp_path / ("solo_" + name))] + flags, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines.append(f"{src}\t{tmp_path / ('batch_' + name)}\n")
    (tmp_path / "list.tsv").write_text("".join(lines))
    r = subprocess.run([build.CLI, "--batch", str(tmp_path / "list.tsv")] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "3 graphs in 1 launch" in r.stderr, r.stderr
    for name, _ in FIXTURES:
        assert (tmp_path / ("batch_" + name)).read_bytes() == (tmp_path / ("solo_" + name)).read_bytes(), name
    r = subprocess.run([build.CLI, "--batch", str(tmp_path / "list.tsv"), "-p", "L"], capture_output=True, text=True)
    assert r.returncode != 0 and "--batch" in r.stderr and "-p Y" in r.stderr
    r = subprocess.run([build.CLI, "--batch", str(tmp_path / "list.tsv"), "-p", "Y", "--layout-out", str(tmp_path / "l.tsv")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--layout-out belongs to -p L" in r.stderr


def test_cli_batch_sort_runs_every_refused_graph_alone(tmp_path):
    """The list and flags above plus --hip-flags 4 (GFS_F_NO_FUSE: no fused launch, so no graph may be in a batch): the batch is
    refused item after item until nothing is left, every graph runs alone after that, and writes what its single run writes."""
    from util import cli_solo_and_batch
    build.build_host()
    names = [name for name, _ in FIXTURES]
    flags = ["-p", "Y", "--streams", "1", "--iter-max", "10", "-v", "1", "--hip-flags", "4"]
    solo, r = cli_solo_and_batch(build.CLI, tmp_path, names, flags, layouts=False)
    assert all(s.returncode == 0 for s in solo), [s.stderr for s in solo]
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("runs alone") == len(names) and "in the batch" not in r.stderr, r.stderr
    for name in names:
        assert (tmp_path / ("batch_" + name)).read_bytes() == (tmp_path / ("solo_" + name)).read_bytes(), name
