"""The layout team kernels for 4 to 8 dimensions (sgd_kernels_nd_team_wide.hip): the trip machine of D = 2, 3 — runs of
GFS_F_CHAIN trips, one set of end flips per run, two partners per leader with twin trips, fused short-jump trips with one add
per end — instantiated for D = 4..8 and reached with an explicit GFS_F_BUNDLE(8..64).  Checked against the oracle's sequential
mirror (generic in D), against GPU reference streams for quality, through the CLI and through two ranks; and what stays as it
was: the auto policy keeps reference streams for D >= 4."""
import os
import queue
import subprocess
import time

import numpy as np
import pytest

from util import O, G, P, load, oracle_graph, oracle_params, gaussian_init
from gfasort_amd import hip, quality as Q

pytestmark = pytest.mark.gpu

WIDE = [4, 5, 6, 7, 8]


def _node_slots(g):
    """The product's internal node layout (first-visit path order): the bundled sampler aligns its runs to the 64-B lines of
    the coordinate planes, so the mirror needs it."""
    from gfasort_amd.distributed import path_order_layout
    return path_order_layout(g)


def _mirror_chain(B):
    """The product's default run length in trips for layouts (GFS_F_CHAIN auto): 16 at B = 64, else one trip per run."""
    return 16 if B == 64 else 1


def _mirror_partners(B):
    """The product's partner draws per leader for layouts of >= 2 dimensions: two at B = 64 unless GFS_F_ONE_PARTNER, else one."""
    return 2 if B == 64 else 1


def _bubble_gfa(g, path):
    first = g.path_first_step.astype(int)
    with open(path, "w") as fh:
        fh.write("H\tVN:Z:1.0\n")
        fh.write("".join(f"S\t{i}\t{'A' * l}\n" for i, l in zip(g.node_ids.tolist(), g.node_len.tolist())))
        for pth, name in enumerate(g.path_names):
            fh.write(f"P\t{name}\t" + ",".join(f"{i}+" for i in g.step_node_id[first[pth]:first[pth + 1]].tolist()) + "\t*\n")


# ---- a. the sampler: trace = mirror ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dims", [(8, 4), (16, 5), (32, 6), (64, 7), (64, 8)])
def test_wide_layout_sampler_trace_matches_oracle_mirror(B, dims):
    g = load("DRB1-3123.gfa")
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = 4
    p.min_term_updates = 60000
    T, K = 256, 64
    og, op = oracle_graph(g), oracle_params(p)
    c0 = gaussian_init(g, dims, 11)
    c_ref = c0.copy()
    st_o = O.State(og, op, dims=dims, n_streams=T, trace_per_stream=K, bundle=B, node_slots=_node_slots(g), chain=_mirror_chain(B),
                   partners=_mirror_partners(B))
    st_o.run(c_ref)
    so = st_o.stats()
    ctx = hip.Context(g)
    assert ctx.setup_nd(p, hip.make_config(n_streams=T, trace_per_stream=K, flags=hip.F_BUNDLE(B))) == 0
    ctx.upload(c0)
    ctx.run()
    tr, counts = ctx.trace()
    hst = ctx.stats()
    assert hst.bundle == B and hst.term_updates == so.term_updates == 5 * p.min_term_updates and hst.attempts == so.attempts
    tr_ref = st_o.trace.reshape(T, K)
    assert np.array_equal(tr["i"], tr_ref["i"]) and np.array_equal(tr["j"], tr_ref["j"])
    assert np.array_equal(tr["d_ij"].view(np.uint64), tr_ref["d_ij"].view(np.uint64))
    assert np.isfinite(ctx.download()).all()
    ctx.close()


# ---- b. one wave in the fused pooled launch: coordinates bit for bit = mirror ------------------------------------------
_ONE_WAVE = [(d, 2, True) for d in WIDE] + [(d, pt, tw) for d in (4, 8) for pt, tw in ((2, False), (1, True))]


@pytest.mark.parametrize("dims,partners,twin", _ONE_WAVE)
def test_wide_layout_team_kernel_single_wave_coords_equal_the_oracle_mirror(dims, partners, twin):
    g = G.synth_windows(40_000, 8, 20_000, 12)
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = 6
    p.min_term_updates = 150_000
    og, op = oracle_graph(g), oracle_params(p)
    c0 = gaussian_init(g, dims, 5)
    c_ref = c0.copy()
    st_o = O.State(og, op, dims=dims, n_streams=64, bundle=64, node_slots=_node_slots(g), chain=_mirror_chain(64),
                   partners=partners, twin_trip=twin)
    st_o.run(c_ref)
    so = st_o.stats()
    ctx = hip.Context(g)
    ctx.setup_nd(p, hip.make_config(n_streams=64, flags=hip.F_BUNDLE(64) | (0 if partners == 2 else hip.F_ONE_PARTNER) |
                                    (0 if twin else hip.F_DBG_NO_TWIN_TRIP)))
    ctx.upload(c0)
    ctx.run()
    hst = ctx.stats()
    c = ctx.download()
    ctx.close()
    assert hst.bundle == 64 and hst.launches == 1
    assert (hst.term_updates, hst.attempts) == (so.term_updates, so.attempts) and hst.term_updates == 7 * 150_000
    assert np.array_equal(c.view(np.uint64), np.ascontiguousarray(c_ref).ravel().view(np.uint64))


# ---- c. the fused launch = one launch per iteration ---------------------------------------------------------------------
@pytest.mark.parametrize("dims", [4, 8])
def test_wide_fused_layout_launch_equals_per_iteration_launches_on_one_wave(dims):
    g = G.synth_windows(40_000, 8, 20_000, 12)
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = 9
    p.min_term_updates = 150_000
    c0 = gaussian_init(g, dims, 5)
    out = []
    # (and the kernels' other forms, bit for bit the same on one wave: fixed quotas — one wave's is the whole iteration, in the
    # pool's chunks — and tables read from global memory)
    others = (hip.F_DBG_FREE_RUNNING, hip.F_NO_LDS_TABLES, hip.F_NO_LDS_TABLES | hip.F_DBG_FREE_RUNNING, hip.F_NO_LDS_TABLES | hip.F_NO_FUSE)
    for extra in (0, hip.F_NO_FUSE) + others:
        ctx = hip.Context(g)
        ctx.setup_nd(p, hip.make_config(n_streams=64, flags=hip.F_BUNDLE(64) | extra))
        ctx.upload(c0)
        ctx.run()
        out.append((ctx.download(), ctx.stats()))
        ctx.close()
    for (c, s), launches in zip(out[2:], (1, 1, 1, 10)):
        assert s.launches == launches and (s.term_updates, s.attempts) == (out[1][1].term_updates, out[1][1].attempts)
        assert np.array_equal(c.view(np.uint64), out[1][0].view(np.uint64))
    (cf, sf), (cu, su) = out[:2]
    assert (sf.launches, su.launches) == (1, 10) and sf.iterations == su.iterations == 10
    assert (sf.term_updates, sf.attempts) == (su.term_updates, su.attempts) and sf.term_updates == 10 * p.min_term_updates
    assert np.array_equal(cf.view(np.uint64), cu.view(np.uint64))


# ---- d. full width -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", WIDE)
def test_wide_layout_full_width_exact_update_count(dims):
    from gfasort_amd import sgd as S
    g = G.synth_bubbles(20_000, 16, 5)
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    c0 = S.default_layout_init(g, dims, p.seed)
    rc, c, st = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(flags=hip.F_BUNDLE(64)))
    assert rc == 0 and st.bundle == 64 and st.launches == 1
    assert st.term_updates == (p.iter_max + 1) * p.min_term_updates
    assert np.isfinite(c).all()


# ---- e. quality against GPU reference streams (the thresholds of tests/test_gpu_quality.py _compare_layout) -------------
def _layout_profile(g, c, dims):
    _, rms, cnt = Q.stress_by_scale(g, c, dims, 1_000_000)
    return rms


def _end_to_end(g, c, dims):
    cc = np.asarray(c).reshape(-1, 2, dims)
    d = np.sqrt(((cc[:, 0, :] - cc[:, 1, :]) ** 2).sum(axis=1))
    err = np.abs(d - g.node_len)
    return float(np.median(err)), float(np.mean(err))


@pytest.mark.parametrize("dims", [4, 8])
def test_wide_layout_team_kernel_against_reference_streams(dims):
    from gfasort_amd import sgd as S
    g = G.synth_bubbles(150_000, 16, 9)                          # 196 875 nodes, 16 haplotypes
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    og = oracle_graph(g)
    c0 = S.default_layout_init(g, dims, p.seed)
    rc, c_b1, st1 = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(flags=hip.F_BUNDLE(1)))
    assert rc == 0 and st1.bundle == 1
    rc, c_b64, st = hip.path_linear_sgd_layout_raw(g, p, c0, cfg=hip.make_config(flags=hip.F_BUNDLE(64)))
    assert rc == 0 and st.bundle == 64 and st.term_updates == st1.term_updates == (p.iter_max + 1) * p.min_term_updates
    s_ref, s_new = O.layout_stress(og, dims, c_b1, 2_000_000), O.layout_stress(og, dims, c_b64, 2_000_000)
    assert s_new <= 1.10 * s_ref, ("sampled layout stress", s_ref, s_new)
    ratio = _layout_profile(g, c_b64, dims) / _layout_profile(g, c_b1, dims)
    assert float(np.max(ratio)) <= 1.12, ("relative error by octave of path distance", np.round(ratio, 3).tolist())
    (m_ref, a_ref), (m_new, a_new) = _end_to_end(g, c_b1, dims), _end_to_end(g, c_b64, dims)
    assert m_new <= 1.10 * m_ref + 0.02 and a_new <= 1.10 * a_ref + 0.02, ((m_ref, a_ref), (m_new, a_new))


# ---- f. what stays as it was -------------------------------------------------------------------------------------------
def test_wide_layout_auto_policy_keeps_reference_streams():
    g = G.synth_bubbles(20_000, 16, 5)                           # 26 250 nodes: the auto policy picks B = 64 for D = 2, 3
    assert g.n_nodes >= 16384
    p = P.LayoutSGDParams.from_graph(g, 4, 1)
    p.iter_max = 2
    ctx = hip.Context(g)
    assert ctx.setup_nd(p, hip.make_config()) == 0
    assert ctx.stats().bundle == 1
    ctx.close()


@pytest.mark.parametrize("dims,B", [(4, 4), (9, 64), (9, 8)])
def test_wide_layout_refusals(dims, B):
    g = G.synth_bubbles(20_000, 16, 5)
    p = P.LayoutSGDParams.from_graph(g, 4, 1)
    p.dimensions = dims
    ctx = hip.Context(g)
    with pytest.raises(hip.GfsError) as e:
        ctx.setup_nd(p, hip.make_config(flags=hip.F_BUNDLE(B)))
    assert e.value.code == -5                                    # GFS_E_UNSUPPORTED
    ctx.close()


# ---- g. the CLI ----------------------------------------------------------------------------------------------------------
def test_cli_wide_layout_with_explicit_bundle(tmp_path):
    from gfasort_amd import build as B
    from gfasort_amd.layout import Layout
    B.build_host()
    g = G.synth_bubbles(20_000, 8, 4)
    assert g.n_nodes >= 16384
    src, o, tsv = str(tmp_path / "b.gfa"), str(tmp_path / "o.gfa"), str(tmp_path / "t.tsv")
    _bubble_gfa(g, src)
    r = subprocess.run([B.CLI, "-i", src, "-o", o, "-p", "L", "--dimensions", "4", "--bundle", "64", "--layout-out", tsv, "-v", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "(bundle 64)" in r.stderr, r.stderr
    with open(tsv) as fh:
        lay = Layout.read_tsv(fh)
    assert (lay.dimensions, lay.num_nodes) == (4, g.n_nodes) and np.isfinite(lay.coords).all()


# ---- h. two ranks on one GPU over gloo, D = 4 at B = 64 -----------------------------------------------------------------
def _mp_rank_wide(rank, world, port, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gfasort_amd.distributed import RankDriver
    from gfasort_amd import sgd as S
    g = G.synth_bubbles(20000, 16, 5)
    p = P.LayoutSGDParams.from_graph(g, 4, 1)
    r = RankDriver(g, p, rank, world, dims=4, device_index=0, dist=dist, merge_every=2, flags=hip.F_BUNDLE(64))
    r.set_positions(S.default_layout_init(g, 4, p.seed).ravel())
    r.run()
    torch.cuda.synchronize()
    c = r.positions_numpy()
    st = r.stats()
    cs = [torch.zeros(c.shape[0], dtype=torch.float64) for _ in range(world)]
    dist.all_gather(cs, torch.from_numpy(c))
    info = torch.tensor([float(st.term_updates), float(st.bundle)], dtype=torch.float64)
    infos = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(infos, info)
    if rank == 0:
        out.put((c, [t.numpy() for t in cs], [t.numpy() for t in infos]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_layout_4d_bundle_64():
    import socket
    import torch.multiprocessing as mp
    from gfasort_amd import sgd as S
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_mp_rank_wide, args=(r, 2, port, out)) for r in range(2)]
    for pr in procs:
        pr.start()
    deadline = time.monotonic() + 300
    while True:                                                  # (a rank that fails ends the wait, not the deadline)
        try:
            c, cs, infos = out.get(timeout=5)
            break
        except queue.Empty:
            failed = [pr.exitcode for pr in procs if pr.exitcode not in (None, 0)]
            if failed or time.monotonic() > deadline:
                for pr in procs:
                    pr.kill()
                pytest.fail(f"ranks ended without a result: exit codes {[pr.exitcode for pr in procs]}")
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    g = G.synth_bubbles(20000, 16, 5)
    p = P.LayoutSGDParams.from_graph(g, 4, 1)
    assert [int(i[1]) for i in infos] == [64, 64]
    assert np.array_equal(cs[0], cs[1]) and sum(i[0] for i in infos) == (p.iter_max + 1) * p.min_term_updates
    og = oracle_graph(g)
    c0 = S.default_layout_init(g, 4, p.seed)
    s0 = O.layout_stress(og, 4, c0, 100000)
    s2 = O.layout_stress(og, 4, c.reshape(-1, 2, 4), 100000)
    assert np.isfinite(c).all() and s2 < 0.1 * s0, (s0, s2)
