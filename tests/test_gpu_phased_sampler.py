"""GFS_F_PHASED (K1e, sgd_kernels_1d_phased.hip): the team sampler at B = 64 outside a window of iterations, reference streams
inside it, one RNG state per lane throughout.  Contract: the oracle's gfo_state at bundle 64 whose bundle is
switched to 1 for the window's iterations and back; launch forms, exact counts, quality at the reference's default schedule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from util import O, G, P, DATA, load, oracle_graph, oracle_params
from gfasort_amd import build as B
from gfasort_amd import hip
from test_gpu_parity import _node_slots, _mirror_chain, _ygs
from test_gpu_quality import _compare

pytestmark = pytest.mark.gpu


def _set_bundle(st_o, b):
    assert O.lib().gfo_state_set_bundle(st_o.h, C.c_uint64(b)) == 0


def _mirror(g, p, T, window, x, trace_per_stream=0):
    st_o = O.State(oracle_graph(g), oracle_params(p), n_streams=T, trace_per_stream=trace_per_stream, bundle=64,
                   node_slots=_node_slots(g), chain=_mirror_chain(64), partners=2)
    for k in range(p.iter_max + 1):
        _set_bundle(st_o, 1 if window[0] <= k < window[1] else 64)
        st_o.run_iteration(k, x)
    return st_o


def _phased(g, p, T, window, extra=0, trace_per_stream=0):
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(n_streams=T, trace_per_stream=trace_per_stream, flags=hip.F_PHASED | hip.F_BUNDLE(64) | extra))
    assert ctx.phase_window(*window) == tuple(window)
    ctx.upload(hip.init_positions(g))
    ctx.run()
    return ctx


def test_sampling_contract_at_full_width_equals_the_oracle_with_its_bundle_switched():
    """4096 streams, per-iteration launches (traces): a window from the heating half into the cooling half (first_cooling = 5):
    a pass left over when the window begins is kept, and dropped after it when the cooling flag changed."""
    g = load("DRB1-3123.gfa")
    p = _ygs(g, 10)
    T, K = 4096, 64
    p.min_term_updates = 4 * T
    window = (4, 8)
    x_ref = O.init_positions(oracle_graph(g))
    st_o = _mirror(g, p, T, window, x_ref, trace_per_stream=K)
    so = st_o.stats()
    ctx = _phased(g, p, T, window, trace_per_stream=K)
    tr, counts = ctx.trace()
    hst = ctx.stats()
    ctx.close()
    assert hst.bundle == 64 and hst.launches == p.iter_max + 1
    assert hst.term_updates == so.term_updates == (p.iter_max + 1) * p.min_term_updates and hst.attempts == so.attempts
    tr_ref = st_o.trace.reshape(T, K)
    assert np.array_equal(tr["i"], tr_ref["i"]) and np.array_equal(tr["j"], tr_ref["j"])
    assert np.array_equal(tr["d_ij"].view(np.uint64), tr_ref["d_ij"].view(np.uint64))


def _wave_graph(graph):
    return G.synth_windows(40_000, 8, 20_000, 12) if graph == "windows" else G.synth_bubbles(30_000, 8, 3)


def _wave_params(g):
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = 8
    p.min_term_updates = 200_000
    return p


@pytest.mark.parametrize("graph", ["windows", "bubbles"])
def test_empty_window_single_wave_equals_the_team_kernels_oracle_mirror(graph):
    g = _wave_graph(graph)
    p = _wave_params(g)
    x_ref = O.init_positions(oracle_graph(g))
    so = _mirror(g, p, 64, (0, 0), x_ref).stats()
    ctx = _phased(g, p, 64, (0, 0))
    hst, x = ctx.stats(), ctx.download()
    ctx.close()
    assert hst.launches == 1
    assert (hst.term_updates, hst.attempts) == (so.term_updates, so.attempts) and hst.term_updates == 9 * 200_000
    assert np.array_equal(x.view(np.uint64), x_ref.view(np.uint64))


@pytest.mark.parametrize("graph", ["windows", "bubbles"])
def test_whole_schedule_window_single_wave_equals_fused_reference_streams(graph):
    g = _wave_graph(graph)
    p = _wave_params(g)
    ctx = _phased(g, p, 64, (0, p.iter_max + 1))
    hst, x = ctx.stats(), ctx.download()
    ctx.close()
    rc, x_b1, s1 = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=64, flags=hip.F_BUNDLE(1)))
    assert rc == 0 and s1.bundle == 1 and s1.launches == 1 and hst.launches == 1
    assert (hst.term_updates, hst.attempts) == (s1.term_updates, s1.attempts) and hst.term_updates == 9 * 200_000
    assert np.array_equal(x.view(np.uint64), x_b1.view(np.uint64))


@pytest.mark.parametrize("graph", ["windows", "bubbles"])
def test_fused_equals_per_iteration_launches_single_wave(graph, monkeypatch):
    """One wave, a window across the cooling switch (first_cooling = 4).  The per-iteration form runs K1 for a window iteration,
    in which every lane works through its whole quota in lockstep trips; the fused launch deals a window iteration out in chunks
    of REF_CHUNK_PER_LANE terms per lane, and the wave meets at every chunk's end.  With rejections the lanes' terms then
    interleave differently (lane a's 17th term runs after every lane's 16th instead of beside lane b's 17th), which on shared
    nodes changes the rounding: the two forms are bit for bit the same where one chunk covers a lane's quota, which the probe
    knob GFS_DBG_REF_CHUNK provides here (3 125 terms per lane and iteration)."""
    monkeypatch.setenv("GFS_DBG_REF_CHUNK", "4096")
    g = _wave_graph(graph)
    p = _wave_params(g)
    window = (3, 7)
    out = []
    for extra, want in ((0, 1), (hip.F_NO_FUSE, 9), (hip.F_NO_LDS_TABLES, 1)):      # (the last: K1e reading its tables from global memory)
        ctx = _phased(g, p, 64, window, extra)
        hst, x = ctx.stats(), ctx.download()
        ctx.close()
        assert hst.launches == want and hst.term_updates == 9 * 200_000
        out.append((x, hst))
    (xf, sf), (xu, su), (xg, sg) = out
    assert sf.attempts == su.attempts == sg.attempts
    assert np.array_equal(xf.view(np.uint64), xu.view(np.uint64)) and np.array_equal(xg.view(np.uint64), xu.view(np.uint64))
    # and both draw what the oracle with its bundle switched for the window draws (its positions differ: its reference streams
    # take one attempt each in turn, 64 lanes of a wave take theirs at once)
    x_ref = O.init_positions(oracle_graph(g))
    so = _mirror(g, p, 64, window, x_ref).stats()
    assert (so.term_updates, so.attempts) == (sf.term_updates, sf.attempts)


def test_exact_counts_at_full_width_and_run_range_lists():
    g = G.synth_windows(50_000, 8, 25_000, 6)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = 20
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(flags=hip.F_PHASED))
    assert ctx.phase_window() == hip.phase_window(p)
    b, e = ctx.phase_window()
    assert 0 < b < e <= 21
    ctx.init_positions()
    ctx.run()
    st = ctx.stats()
    assert st.bundle == 64 and st.n_streams % 64 == 0 and st.launches == 1 and st.term_updates == 21 * p.min_term_updates
    l0 = st.launches                                                          # (launches: over the context's life)
    ctx.setup_1d(p, hip.make_config(flags=hip.F_PHASED))
    ctx.upload(hip.init_positions(g))
    ctx.run_range([0, 1, 2, 3, 4])
    ctx.run_range([5, 6, 7, 20, 20, 0, 1])
    ctx.run_range(list(range(8, 21)))
    ctx.synchronize()
    st = ctx.stats()
    assert st.launches - l0 == 3 and st.iterations == 25 and st.term_updates == 25 * p.min_term_updates
    assert np.isfinite(ctx.download()).all()
    with pytest.raises(Exception):
        ctx.run_range([21])
    # a schedule longer than one fused launch covers (4096 iterations)
    p.iter_max = 5000
    p.min_term_updates = 50_000
    l0 = st.launches
    ctx.setup_1d(p, hip.make_config(flags=hip.F_PHASED))
    ctx.init_positions()
    ctx.run()
    st = ctx.stats()
    assert st.launches - l0 == 2 and st.term_updates == 5001 * 50_000
    assert np.isfinite(ctx.download()).all()
    ctx.close()


def _run(ctx, p, flags):
    ctx.setup_1d(p, hip.make_config(flags=flags))
    ctx.init_positions()
    ctx.run()
    return ctx.download(), ctx.stats()


@pytest.mark.parametrize("shuffle_seed", [None, 17])
def test_phased_sampler_at_parity_on_drb1_tiled_in_series_at_the_default_schedule(shuffle_seed):
    """The graph on which the default sampler is behind at --iter-max 100 (test_gpu_quality.py
    test_default_flags_on_drb1_tiled_in_series: x1.65 at path distance 1): the phased sampler against reference streams at
    the ORDINARY thresholds, and at --iter-max 300."""
    g = G.tile_series(load("DRB1-3123.gfa"), 120, shuffle_seed=shuffle_seed)
    og = oracle_graph(g)
    ctx = hip.Context(g)
    for iter_max in (100, 300) if shuffle_seed is None else (100,):
        p = P.YgsParams.from_graph(g, 0, 1).path_sgd
        p.iter_max = iter_max
        x_ph, st = _run(ctx, p, hip.F_PHASED)
        assert st.bundle == 64 and st.launches >= 1 and st.term_updates == (iter_max + 1) * p.min_term_updates
        x_b1, st1 = _run(ctx, p, hip.F_BUNDLE(1))
        assert st1.bundle == 1 and st1.term_updates == st.term_updates
        _compare(g, og, x_b1, x_ph, f"DRB1 x120 --iter-max {iter_max}, phased sampler vs GPU reference streams")
    ctx.close()


def test_phased_sampler_at_parity_on_a_525k_node_bubble_graph():
    g = G.synth_bubbles(400_000, 24, 6)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    og = oracle_graph(g)
    ctx = hip.Context(g)
    x_ph, st = _run(ctx, p, hip.F_PHASED)
    x_b1, st1 = _run(ctx, p, hip.F_BUNDLE(1))
    ctx.close()
    assert st.bundle == 64 and st1.term_updates == st.term_updates == (p.iter_max + 1) * p.min_term_updates
    _compare(g, og, x_b1, x_ph, "525k bubble graph, phased sampler vs GPU reference streams")


def test_phased_sampler_speed_on_drb1_tiled_in_series():
    g = G.tile_series(load("DRB1-3123.gfa"), 120)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    ctx = hip.Context(g)
    ms = {}
    for name, fl in (("warm-up", hip.F_PHASED), ("warm-up ref", hip.F_BUNDLE(1)), ("phased", hip.F_PHASED), ("ref", hip.F_BUNDLE(1))):
        ctx.setup_1d(p, hip.make_config(flags=fl))
        ctx.init_positions()
        ctx.run()
        ms[name] = ctx.stats().kernel_ms
    ctx.close()
    assert ms["phased"] <= 0.75 * ms["ref"], ms


def test_refusals_and_hook_errors():
    g = G.synth_windows(50_000, 8, 25_000, 6)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = 10
    ctx = hip.Context(g)
    for flags in (hip.F_PHASED | hip.F_BUNDLE(32), hip.F_PHASED | hip.F_BUNDLE(1), hip.F_PHASED | hip.F_BUNDLE(16)):
        with pytest.raises(hip.GfsError) as ei:
            ctx.setup_1d(p, hip.make_config(flags=flags))
        assert ei.value.code == -1
    lp = P.LayoutSGDParams.from_graph(g, 2, 1)
    with pytest.raises(hip.GfsError) as ei:
        ctx.setup_nd(lp, hip.make_config(flags=hip.F_PHASED))
    assert ei.value.code == -1
    ctx.setup_1d(p, hip.make_config())                                        # without the flag
    with pytest.raises(hip.GfsError) as ei:
        ctx.phase_window()
    assert ei.value.code == -4
    ctx.setup_1d(p, hip.make_config(flags=hip.F_PHASED | hip.F_BUNDLE(64)))
    for bad in ((5, 4), (0, 12), (3, -1), (-1, 3)):
        with pytest.raises(hip.GfsError) as ei:
            ctx.phase_window(*bad)
        assert ei.value.code == -1
    assert ctx.phase_window(0, 11) == (0, 11) and ctx.phase_window() == (0, 11)
    ctx.close()


def test_flag_is_a_no_op_where_reference_streams_are_picked():
    g = load("DRB1-3123.gfa")                                                 # 4 955 nodes: the auto policy runs reference streams
    p = _ygs(g, 20)
    # (one stream: reference streams at full width are not deterministic from run to run — their adds race — with or without it)
    rc, x0, s0 = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1))
    rc1, x1, s1 = hip.path_linear_sgd_raw(g, p, cfg=hip.make_config(n_streams=1, flags=hip.F_PHASED))
    assert rc == rc1 == 0 and s0.bundle == s1.bundle == 1 and (s0.term_updates, s0.attempts) == (s1.term_updates, s1.attempts)
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    ctx = hip.Context(g)
    ctx.setup_1d(p, hip.make_config(flags=hip.F_PHASED))
    assert ctx.phase_window() == (0, 21)
    with pytest.raises(hip.GfsError) as ei:
        ctx.phase_window(0, 5)
    assert ei.value.code == -4
    ctx.close()


def test_cli_phased_sampler_recovers_chain_order(tmp_path):
    B.build_host()
    g = G.synth_chain(20000, 1)
    src = tmp_path / "chain.gfa"
    src.write_text(G.synth_to_gfa_text(g))
    o = str(tmp_path / "chain.sorted.gfa")
    r = subprocess.run([B.CLI, "-i", str(src), "-o", o, "-p", "Y", "-v", "2", "--phased-sampler"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert "(bundle 64)" in r.stderr and "phased sampler: reference streams in iterations [" in r.stderr, r.stderr
    g2 = G.load_gfa(o)
    lens_by_old_id = np.empty(20001, dtype=np.int64)
    lens_by_old_id[g.node_ids.astype(np.int64)] = g.node_len
    chain = lens_by_old_id[1:]
    assert np.array_equal(g2.node_len, chain) or np.array_equal(g2.node_len, chain[::-1])
    ids = g2.step_node_id.astype(np.int64)
    assert np.array_equal(ids, np.arange(1, 20001)) or np.array_equal(ids, np.arange(20000, 0, -1))
