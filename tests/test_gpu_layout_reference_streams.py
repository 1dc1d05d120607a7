"""The reference-stream layout kernels K2 (sgdnd_kernel<D>) and K2d (sgdnd_fused_kernel<D>) at EVERY dimension 1..8.

They are what `-p L --dimensions 4..8` runs by default and the yardstick of test_gpu_layout_wide.py; before this file only
D = 2, 3 were ever compared with anything.  "Oracle" is O.sgd_nd / O.State (deterministic mode), "replay" is
util.replay_layout_trace — the layout update restated from sgd.rs:1085-1149 in Python floats, which
test_layout_update_restatement.py ties to the oracle on the CPU.  Everything bit-exact is compared as uint64 views, with
term_updates and attempts.

The replay has no crowding term; one-stream runs have kshift = floor(log2(n_steps / 2)) + 2, above every exponent of these
fixtures.  That premise is asserted (np_crowding on the host, gfs_ctx_debug_kshift as a query on the device).

Kernel mutations tried on a scratch build (valid, in-bounds, wrong-answer code; not committed) and what caught them are
listed in HISTORY.md (R6).
"""
import math
import os
import subprocess

import numpy as np
import pytest

from util import (O, G, P, DATA, load, oracle_graph, oracle_params, gaussian_init, replay_layout_trace, np_crowding,
                  self_loop_graph, absent_node_graph, reverse_short_paths_graph, single_stream_kshift)
from gfasort_amd import build as B
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

ALL_DIMS = [1, 2, 3, 4, 5, 6, 7, 8]


def _layout_params(g, dims, iter_max=None, min_term_updates=None):
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    if iter_max is not None:
        p.iter_max = iter_max
    if min_term_updates is not None:
        p.min_term_updates = min_term_updates
    return p


def _oracle_one_stream(g, p, c0):
    c_ref = c0.copy()
    rc, st, _ = O.sgd_nd(oracle_graph(g), oracle_params(p), c_ref, n_streams=1)
    assert rc == 0 and st.term_updates == (p.iter_max + 1) * p.min_term_updates
    return c_ref, st


def _gpu_one_stream(g, p, c0, flags, want_launches):
    rc, c, hst = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(n_streams=1, flags=flags))
    assert rc == 0 and hst.bundle == 1 and hst.n_streams == 1
    assert hst.launches == want_launches, (hst.launches, want_launches)      # documents which kernel ran: 1 = K2d, else K2
    return c, hst


def _same(c, hst, c_ref, st):
    assert (hst.term_updates, hst.attempts) == (st.term_updates, st.attempts)
    assert np.array_equal(c.view(np.uint64), c_ref.view(np.uint64)), _first_difference(c, c_ref)


def _first_difference(c, c_ref):
    bad = np.flatnonzero(c.view(np.uint64) != c_ref.view(np.uint64))
    return f"{bad.shape[0]} of {c.shape[0]} words differ, first at flat index {int(bad[0])}" if bad.shape[0] else "equal"


def _gpu_traced_unfused(g, p, c0):
    """K2 (a trace disables fusing, capi.hip can_fuse) on one stream with every update traced.  Returns (coords, trace, stats,
    kshift)."""
    total = (p.iter_max + 1) * p.min_term_updates
    ctx = hip.Context(g)
    try:
        assert ctx.setup_nd(p, hip.make_config(n_streams=1, flags=hip.F_NO_FUSE, trace_per_stream=total)) == 0
        kshift = ctx.kshift()
        ctx.upload(c0)
        ctx.run()
        tr, counts = ctx.trace()
        hst = ctx.stats()
        c = ctx.download()
    finally:
        ctx.close()
    assert hst.launches == p.iter_max + 1 and hst.bundle == 1
    assert int(counts[0]) == total == hst.term_updates and tr.shape == (1, total)
    return c, tr[0], hst, kshift


def _assert_no_crowding(g, kshift):
    _, _, a, _ = np_crowding(g)
    assert kshift == single_stream_kshift(g) and a.max() < kshift, (int(a.max()), kshift)


# ---- a. one stream, every D, both launch forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ALL_DIMS)
def test_one_stream_fused_and_unfused_equal_the_oracle_and_the_replay(dims):
    """K2d (one launch) and K2 (one launch per iteration) on one stream equal the oracle bit for bit at D = 1..8, across the
    cooling switch.  The unfused kernel's own trace, fed to the replay, gives its own coordinates: that ties the kernel's
    arithmetic to the restatement of sgd.rs without the oracle in between.  A trace disables fusing (capi.hip can_fuse), so
    the fused form is tied to the restatement through the oracle only (and through the unfused form it equals)."""
    g = load("DRB1-3123.gfa")
    p = _layout_params(g, dims, 5, 12000)
    c0 = gaussian_init(g, dims, 7)
    c_ref, st = _oracle_one_stream(g, p, c0)
    c, hst = _gpu_one_stream(g, p, c0, 0, 1)
    _same(c, hst, c_ref, st)
    c, hst = _gpu_one_stream(g, p, c0, hip.F_NO_FUSE, p.iter_max + 1)
    _same(c, hst, c_ref, st)
    ct, tr, tst, kshift = _gpu_traced_unfused(g, p, c0)
    _assert_no_crowding(g, kshift)
    _same(ct, tst, c_ref, st)
    c_replay = replay_layout_trace(c0, dims, tr, hip.sgd_schedule(p), p.min_term_updates)
    assert np.array_equal(ct.view(np.uint64), c_replay.view(np.uint64)), _first_difference(ct, c_replay)


# ---- b. the four <LDS_TABLES, ATOMIC_LOADS> forms ------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, hip.F_PLAIN_LOADS, hip.F_NO_LDS_TABLES, hip.F_PLAIN_LOADS | hip.F_NO_LDS_TABLES])
@pytest.mark.parametrize("dims", [1, 5, 8])
def test_template_forms_equal_the_oracle(dims, flags):
    """GFS_F_PLAIN_LOADS makes atomic_loads false, which also turns fusing off (capi.hip can_fuse): those two forms are K2
    <LDS, false>, one launch per iteration; without it K2d<LDS> runs in one launch, and K2<LDS, true> under GFS_F_NO_FUSE."""
    g = load("DRB1-3123.gfa")
    p = _layout_params(g, dims, 4, 10000)
    c0 = gaussian_init(g, dims, 7)
    c_ref, st = _oracle_one_stream(g, p, c0)
    plain = bool(flags & hip.F_PLAIN_LOADS)
    c, hst = _gpu_one_stream(g, p, c0, flags, p.iter_max + 1 if plain else 1)
    _same(c, hst, c_ref, st)
    if not plain:
        c, hst = _gpu_one_stream(g, p, c0, flags | hip.F_NO_FUSE, p.iter_max + 1)
        _same(c, hst, c_ref, st)


# ---- c. degenerate starts and graphs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ALL_DIMS)
def test_all_zero_start_equals_the_oracle_and_the_replay(dims):
    """Every pair's first touch has mag_sq == 0: deltas[0] = 1e-9 (sgd.rs:1116-1119)."""
    g = load("DRB1-3123.gfa")
    p = _layout_params(g, dims, 3, 20000)
    c0 = np.zeros(g.n_nodes * 2 * dims, dtype=np.float64)
    c_ref, st = _oracle_one_stream(g, p, c0)
    assert c_ref.any() and np.isfinite(c_ref).all()
    c, hst = _gpu_one_stream(g, p, c0, 0, 1)
    _same(c, hst, c_ref, st)
    ct, tr, tst, kshift = _gpu_traced_unfused(g, p, c0)
    _assert_no_crowding(g, kshift)
    _same(ct, tst, c_ref, st)
    c_replay = replay_layout_trace(c0, dims, tr, hip.sgd_schedule(p), p.min_term_updates)
    assert np.array_equal(ct.view(np.uint64), c_replay.view(np.uint64)), _first_difference(ct, c_replay)


@pytest.mark.parametrize("dims", ALL_DIMS)
def test_self_loop_path_equals_the_oracle(dims):
    """Terms with idx_i == idx_j: the reference's second store wins (sgd.rs:1143-1149); the kernels issue one add (`same`)."""
    g = self_loop_graph()
    p = _layout_params(g, dims, 20)
    c0 = gaussian_init(g, dims, 3)
    c_ref = c0.copy()
    total = (p.iter_max + 1) * p.min_term_updates
    rc, st, tr = O.sgd_nd(oracle_graph(g), oracle_params(p), c_ref, n_streams=1, trace_per_stream=total)
    assert rc == 0 and int((tr["i"] == tr["j"]).sum()) >= 1
    for flags, want in ((0, 1), (hip.F_NO_FUSE, p.iter_max + 1)):
        c, hst = _gpu_one_stream(g, p, c0, flags, want)
        _same(c, hst, c_ref, st)


@pytest.mark.parametrize("graph", ["absent_node", "reverse_short_paths"])
@pytest.mark.parametrize("dims", [1, 4, 8])
def test_absent_nodes_reverse_steps_and_short_paths_equal_the_oracle(dims, graph):
    """path_len - pos[s] for a path's last step, the 0xFFFFFFFF rejection after both flips have been drawn (the generator's
    state must move as the reference's does), reverse steps' end selection, paths shorter than the sampler's jump."""
    if graph == "absent_node":
        g = absent_node_graph()
        assert int((g.step_node == G.NO_NODE).sum()) == 1
        p = _layout_params(g, dims)
    else:
        g = reverse_short_paths_graph()
        p = _layout_params(g, dims, 4)
    c0 = gaussian_init(g, dims, 3)
    c_ref, st = _oracle_one_stream(g, p, c0)
    assert st.attempts > st.term_updates
    for flags, want in ((0, 1), (hip.F_NO_FUSE, p.iter_max + 1)):
        c, hst = _gpu_one_stream(g, p, c0, flags, want)
        _same(c, hst, c_ref, st)


# ---- d. the sampler of every instantiation at full width -------------------------------------------------------------------
@pytest.mark.parametrize("dims", [1, 4, 5, 6, 7, 8])
def test_sampler_trace_full_width(dims):
    """The first 64 terms of each of 2048 streams (i, j, d_ij bits), updates and attempts equal the oracle's.  The sampler does
    not read coordinates, so this is exact under races (test_gpu_parity.py test_sampler_trace_full_width_nd is D = 2)."""
    g = load("DRB1-3123.gfa")
    p = _layout_params(g, dims, 4, 100000)
    T, K = 2048, 64
    c0 = gaussian_init(g, dims, 7)
    c_ref = c0.copy()
    rc, st, tr_ref = O.sgd_nd(oracle_graph(g), oracle_params(p), c_ref, n_streams=T, trace_per_stream=K)
    assert rc == 0
    ctx = hip.Context(g)
    try:
        assert ctx.setup_nd(p, hip.make_config(n_streams=T, trace_per_stream=K)) == 0
        ctx.upload(c0)
        ctx.run()
        tr, counts = ctx.trace()
        hst = ctx.stats()
    finally:
        ctx.close()
    assert hst.bundle == 1 and (hst.term_updates, hst.attempts) == (st.term_updates, st.attempts)
    assert (counts == K).all()
    tr_ref = tr_ref.reshape(T, K)
    assert np.array_equal(tr["i"], tr_ref["i"]) and np.array_equal(tr["j"], tr_ref["j"])
    assert np.array_equal(tr["d_ij"].view(np.uint64), tr_ref["d_ij"].view(np.uint64))


# ---- e. nothing is lost under contention -----------------------------------------------------------------------------------
def _no_repeat_inside_a_path(g):
    first = g.path_first_step.astype(np.int64)
    path_of = np.repeat(np.arange(first.shape[0] - 1), np.diff(first))
    present = g.step_node != G.NO_NODE
    key = path_of[present] * (g.n_nodes + 1) + g.step_node[present].astype(np.int64)
    return np.unique(key).shape[0] == key.shape[0]


@pytest.mark.parametrize("launch", ["fused", "unfused", "ragged"])
@pytest.mark.parametrize("dims", [1, 2, 4, 8])
def test_coordinate_sums_are_conserved_at_full_width(dims, launch):
    """Every term adds -r_d to one word and +r_d to another, so the sum of each dimension over all node ends changes only by
    the rounding of the adds: |fsum(after[:, k]) - fsum(before[:, k])| <= 2 U 2^-53 M_k, the worst case of 2 U correctly
    rounded adds on words of magnitude <= M_k (U = term_updates, M_k = max |coordinate| of dimension k before or after;
    math.fsum is exact).  Derived, not tuned; the oracle's own drift is five orders of magnitude inside it, one lost or doubled
    add of a bp-sized term breaks it.  Needs a graph where no path steps on a node twice (an i == j term adds once).
    A non-atomic read-modify-write, a wrong plane stride for some k, an add under a wrong exec mask show up here.
    'ragged' is a fused launch of 1000 streams (no multiple of 64)."""
    g = G.synth_bubbles(20_000, 16, 5)
    assert g.n_nodes == 26250 and _no_repeat_inside_a_path(g)
    p = _layout_params(g, dims, 4)
    before = gaussian_init(g, dims, 7)
    cfg = hip.make_config(n_streams=1000 if launch == "ragged" else 0,
                          flags=hip.F_BUNDLE(1) | (hip.F_NO_FUSE if launch == "unfused" else 0))
    rc, after, st = hip.path_linear_sgd_layout_raw(g, p, before, cfg=cfg)
    assert rc == 0 and st.bundle == 1
    assert st.launches == (p.iter_max + 1 if launch == "unfused" else 1)
    assert st.n_streams == 1000 if launch == "ragged" else st.n_streams >= 1024
    U = (p.iter_max + 1) * p.min_term_updates
    assert st.term_updates == U
    assert np.isfinite(after).all()
    assert not np.array_equal(after, before)
    b, a = before.reshape(-1, dims), after.reshape(-1, dims)
    for k in range(dims):
        drift = abs(math.fsum(a[:, k].tolist()) - math.fsum(b[:, k].tolist()))
        M = max(float(np.abs(b[:, k]).max()), float(np.abs(a[:, k]).max()))
        bound = 2.0 * U * 2.0 ** -53 * M
        print(f"conservation D={dims} {launch} k={k}: drift {drift:.3e} bound {bound:.3e} M {M:.4g} U {U} streams {st.n_streams}")
        assert drift <= bound, (dims, launch, k, drift, bound)


# ---- f. the yardstick of test_gpu_layout_wide.py against the CPU, at full width ----------------------------------------------
QUALITY_SEEDS = [9399220 + 1000 * k for k in range(8)]
QUALITY_STREAMS = 1216                    # what the library picks for DRB1 (one stream per 4 nodes, launch_policy.h auto_stream_count)
QUALITY_PAIRED_SD = {4: 0.02893, 8: 0.02900}      # oracle alone, relative to the mean stress (profiles/r06/quality_margin.log)


@pytest.mark.parametrize("dims", [4, 8])
def test_full_width_quality_matches_the_oracle(dims):
    """GPU reference streams at LayoutSGDParams.from_graph defaults against the oracle's deterministic mode, in the form of
    test_gpu_parity.py test_full_width_drb1_quality_matches_oracle: means of O.layout_stress(., 100000) over seeds,
    |gpu - ref| < m * ref.  One run's stress has a relative sd of 7-8 % over seeds, so both sides use the same 8 seeds
    (QUALITY_SEEDS, the sampler's; the start is gaussian_init(seed 7) throughout) and the same 1216 streams — stream t then
    draws the same terms on both sides and only the interleaving differs — and m is four standard errors of the mean paired
    difference, 4 sd / sqrt(8).  sd is measured FROM THE ORACLE ALONE (tests/measure_layout_quality_margin.py, no GPU):
    round-robin over all 1216 streams against the two halves of the streams run one after the other in every iteration, same
    seeds.  Measured: sd of the paired relative difference 0.02893 at D = 4, 0.02900 at D = 8 (mean -0.0013 at both), so
    m = 0.0409 and 0.0410.  Nothing here is derived from GPU output.  At 1216 streams kshift is 5 and DRB1's largest crowding
    exponent is 4, so the product's crowding rule is idle and the oracle needs none; asserted.
    Both launch forms are held to m.  K2 (GFS_F_NO_FUSE) gives every stream the oracle's fixed quota, so the premise "same
    terms, another interleaving" holds exactly there and the attempts are equal (asserted).  K2d, the default, hands out an
    iteration's updates from a work pool (sgd_kernel_common.h ref_pooled_walk): stream t still draws from the same generator,
    but how far it gets in an iteration depends on the race for the pool, so its attempts differ from the oracle's by ~1e-5 of
    the total (seen: 11 198 692 against 11 198 551) and only the update count is asserted."""
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    p = _layout_params(g, dims)
    assert (p.iter_max, p.min_term_updates) == (30, 350590)
    c0 = gaussian_init(g, dims, 7)
    ctx = hip.Context(g)
    try:
        assert ctx.setup_nd(p) == 0
        assert ctx.stats().n_streams == QUALITY_STREAMS and ctx.stats().bundle == 1      # the default is what is measured
        assert np_crowding(g)[2].max() < ctx.kshift()
    finally:
        ctx.close()
    s_ref, s_gpu = [], {"fused": [], "unfused": []}
    for seed in QUALITY_SEEDS:
        p.seed = seed
        c_ref = c0.copy()
        rc, st, _ = O.sgd_nd(og, oracle_params(p), c_ref, n_streams=QUALITY_STREAMS)
        assert rc == 0
        s_ref.append(O.layout_stress(og, dims, c_ref, 100000))
        for form, flags, launches in (("fused", 0, 1), ("unfused", hip.F_NO_FUSE, p.iter_max + 1)):
            rc, c, hst = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(n_streams=QUALITY_STREAMS, flags=flags))
            assert rc == 0 and hst.bundle == 1 and hst.launches == launches and hst.n_streams == QUALITY_STREAMS
            assert hst.term_updates == st.term_updates
            if form == "unfused":
                assert hst.attempts == st.attempts                 # fixed quotas: stream t draws the same terms on both sides
            s_gpu[form].append(O.layout_stress(og, dims, c, 100000))
    m = 4.0 * QUALITY_PAIRED_SD[dims] / math.sqrt(len(QUALITY_SEEDS))
    ref = float(np.mean(s_ref))
    for form, vals in s_gpu.items():
        print(f"quality D={dims} {form}: ref {np.round(s_ref, 4).tolist()} gpu {np.round(vals, 4).tolist()} "
              f"means {ref:.5f} {np.mean(vals):.5f} rel diff {(np.mean(vals) - ref) / ref:+.4f} m {m:.4f}")
    for form, vals in s_gpu.items():
        assert abs(np.mean(vals) - ref) < m * ref, (form, s_ref, vals)


# ---- g. the default path end to end ------------------------------------------------------------------------------------------
def test_cli_default_five_dimensional_layout(tmp_path):
    """`gfasort_hip -p L --dimensions 5` is sgdnd_fused_kernel<5, true> (the auto policy keeps reference streams for D >= 4 and
    gfs_ctx_run_range fuses them).  Then with --streams 1: the start is gfs_init_layout, which O.init_layout restates, and the
    TSV prints the shortest decimal that round-trips, so the coordinates read back equal the oracle's run bit for bit."""
    from gfasort_amd.layout import Layout
    B.build_host()
    src = os.path.join(DATA, "DRB1-3123.gfa")
    g = load("DRB1-3123.gfa")
    og = oracle_graph(g)
    o, tsv = str(tmp_path / "o.gfa"), str(tmp_path / "l.tsv")
    r = subprocess.run([B.CLI, "-i", src, "-o", o, "-p", "L", "--dimensions", "5", "--layout-out", tsv, "-v", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "(bundle 1)" in r.stderr and " in 31 iterations on " in r.stderr, r.stderr
    with open(tsv) as fh:
        lay = Layout.read_tsv(fh)
    assert (lay.dimensions, lay.num_nodes) == (5, 4955) and np.isfinite(lay.coords).all()
    stress = float(r.stderr.split("layout stress:")[1].split()[0])
    assert abs(stress - O.layout_stress(og, 5, lay.coords, 10000)) < 1e-5
    # one stream, a short schedule: bit for bit through the text file
    tsv1 = str(tmp_path / "l1.tsv")
    r = subprocess.run([B.CLI, "-i", src, "-o", o, "-p", "L", "--dimensions", "5", "--layout-out", tsv1, "-v", "1",
                        "--streams", "1", "--layout-iter", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "on 1 streams (bundle 1)" in r.stderr, r.stderr
    with open(tsv1) as fh:
        lay1 = Layout.read_tsv(fh)
    p = _layout_params(g, 5, 2)
    c_ref = O.init_layout(og, 5, p.seed)
    rc, st, _ = O.sgd_nd(og, oracle_params(p), c_ref, n_streams=1)
    assert rc == 0 and f"{st.term_updates} term updates in 3 iterations" in r.stderr, r.stderr
    assert (lay1.dimensions, lay1.num_nodes) == (5, 4955)
    got = np.ascontiguousarray(lay1.coords, dtype=np.float64).reshape(-1)
    assert np.array_equal(got.view(np.uint64), c_ref.view(np.uint64)), _first_difference(got, c_ref)
