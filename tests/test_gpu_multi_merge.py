"""The multi-rank merge (csrc/multi.hip: exchange_snapshot / exchange_prepare / exchange_apply / finish_mask and the host
logic of gfs_rank_*) against the numpy restatement of tests/multi_restatement.py, bit for bit.

An in-process cluster: W hip.Rank objects on device 0, one process, one thread, one reference stream per rank; the test is
the collective.  Per window every rank's exchange buffer, the sum and every rank's replica after the apply are compared;
at the finish every rank's masked vector in device order and the final positions.  The buffers bound into the ranks are
the caller's, allocated through the HIP runtime the library itself is linked to (`Dev`, tests/device_raw.py) and summed on the host in
the payload type: the suite's process cannot also start torch's own copy of the runtime once the library's is in use, so
the tensors of RankDriver are left to the tests that run it in processes of their own (tests/test_gpu_parity.py).

Every comparison is array_equal on the bit patterns: a rank's own updates equal the oracle's at one stream (the control
below and tests/test_gpu_parity.py), and the merge is a cast, a sum made here, one multiply, one divide and one add
without contraction.

The inputs are tests/multi_cases.py; tests/test_multi_restatement_host.py asserts that each reaches its edges."""
import ctypes as C
import threading

import numpy as np
import pytest

import multi_cases as MC
from device_raw import Dev, download as _download, rt as _rt, sync as _sync, upload as _upload
from multi_restatement import bits, hexval
from util import O, oracle_graph, oracle_params
from gfasort_amd import hip
from gfasort_amd.distributed import SHARDING, subgraph

pytestmark = pytest.mark.gpu


def _same(cl, got, want, where, space):
    """array_equal on the bit patterns; a failure names the first differing element as (plane, slot, dense node).
    space: "exchange" ([delta | touched] of the shared elements), "device" (planes x slots) or "abi"."""
    got = np.ascontiguousarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = bits(got), bits(want)
    if np.array_equal(gb, wb):
        return
    bad = np.flatnonzero(gb != wb)
    i = int(bad[0])
    if space == "exchange":
        what = ("delta" if i < cl.total else "touched") + " of (plane, slot, node) " + str(cl.describe(i % cl.total))
    elif space == "device":
        n = cl.g.n_nodes
        what = "(plane, slot, node) " + str((i // n, i % n, int(cl.node_of_slot[i % n])))
    else:
        what = "(plane, slot, node) " + str(cl.describe_abi(i))
    pytest.fail(f"{where}: {bad.shape[0]} of {gb.shape[0]} elements differ, the first is element {i}, {what}: "
                f"got {hexval(got[i])} ({got[i]!r}), want {hexval(want[i])} ({want[i]!r})")


def _ranks(case, cl):
    g, p = MC.graph(case.graph), MC.params(case)
    ranks = [hip.Rank(g, p, case.dims, r, case.world, device=0, sharding=SHARDING[case.sharding], merge_every=case.merge_every,
                      merge_rule=case.merge, payload_f64=case.f64, whole_vector=case.whole_vector,
                      launch=hip.make_config(n_streams=1)) for r in range(case.world)]
    for r, rk in enumerate(ranks):
        info = rk.info()
        assert (int(info.exchange_count), int(info.positions_len), int(info.quota), bool(info.idle)) == \
            (2 * cl.total, g.n_nodes * cl.width, cl.quotas[r], cl.idle[r]), r
        assert int(info.shared_slots) * cl.planes == cl.total
    return ranks


def _close(ranks, buffers=()):
    _sync()
    for rk in ranks:
        rk.close()
    for b in buffers:
        b.free()


def _window(cl, ranks, bufs, rec, name):
    for rk in ranks:
        rk.window_begin(rec["ks"])
    _sync()
    if cl.total:
        got = [b.host() for b in bufs]
        for r in range(cl.world):
            _same(cl, got[r], rec["bufs"][r], f"{name}, rank {r}, buffer before the sum", "exchange")
        s = got[0].copy()
        for r in range(1, cl.world):
            s = s + got[r]
        _same(cl, s, rec["sum"], f"{name}, the summed buffer", "exchange")
        for b in bufs:
            b.set(s)
    for rk in ranks:
        rk.window_end()
    for r, rk in enumerate(ranks):
        _same(cl, rk.get_positions(), rec["x"][r], f"{name}, rank {r}, positions after the apply", "abi")


def _finish(cl, ranks, fulls, rec, name):
    for rk, full in zip(ranks, fulls):
        rk.finish_begin(full.ptr)
    _sync()
    got = [full.host() for full in fulls]
    for r in range(cl.world):
        _same(cl, got[r], rec["masked"][r][cl.abi_of_device], f"{name}, rank {r}, masked vector", "device")
    s = got[0].copy()
    for r in range(1, cl.world):
        s = s + got[r]
    for full in fulls:
        full.set(s)
    for rk, full in zip(ranks, fulls):
        rk.finish_end(full.ptr)
    _sync()
    for r, rk in enumerate(ranks):
        _same(cl, rk.get_positions(), rec["x"], f"{name}, rank {r}, final positions", "abi")


@pytest.mark.parametrize("cid", [c.id for c in MC.CASES])
def test_merge_equals_the_restatement_bit_for_bit(cid):
    case, cl = MC.BY_ID[cid], MC.restated(cid)
    ranks = _ranks(case, cl)
    bufs, fulls = [], []
    try:
        bufs += [Dev(2 * cl.total, np.float64 if case.f64 else np.float32) for _ in ranks] if cl.total else []
        for rk, b in zip(ranks, bufs):
            rk.bind_exchange_buffer(b.ptr)
        fulls += [Dev(cl.g.n_nodes * cl.width, np.float64) for _ in ranks]
        for x in MC.starts(case):
            for rk in ranks:
                rk.set_positions(x)
        wi = fi = 0
        for st in MC.schedule(case):
            if st[0] == "window":
                assert cl.windows[wi]["ks"] == list(st[1])
                _window(cl, ranks, bufs, cl.windows[wi], f"{cid} window {wi} (iterations {list(st[1])})")
                wi += 1
            else:
                _finish(cl, ranks, fulls, cl.finishes[fi], f"{cid} finish {fi}")
                fi += 1
        assert wi == len(cl.windows) and fi == len(cl.finishes)
        assert [int(rk.info().windows) for rk in ranks] == [wi] * case.world
    finally:
        _close(ranks, bufs + fulls)


@pytest.mark.parametrize("cid", ["A-w3-anneal-f32-e1", "D-windows-d2-w3-anneal-f32"])
def test_control_one_shard_alone_equals_the_oracle(cid):
    """Not the merge: one rank's context by itself — the shared layout as node_perm, a stream base that is not its rank's,
    its quota (not min_term_updates) as term_updates_per_iteration, one fused window of three iterations — equals the
    oracle bit for bit.  When this passes and the test above fails, the merge differs, not the shard's run."""
    case, cl = MC.BY_ID[cid], MC.restated(cid)
    g, p, rank = MC.graph(case.graph), MC.params(case), 1
    quota = cl.quotas[rank]
    assert 0 < quota != p.min_term_updates
    sub = subgraph(g, cl.plan.paths_of(rank))
    x0 = np.ascontiguousarray(MC.starts(case)[-1]) if case.dims else O.init_positions(oracle_graph(g))
    st = O.State(oracle_graph(sub), oracle_params(p), dims=case.dims, n_streams=1, stream_base=2, quota_total=quota)
    want = x0.copy()
    for k in (3, 4, 5):
        st.run_iteration(k, want)
    st.close()
    ctx = hip.Context(sub, node_perm=cl.plan.perm)
    try:
        cfg = hip.make_config(n_streams=1, stream_base=2, term_updates_per_iteration=quota)
        assert (ctx.setup_nd(p, cfg) if case.dims else ctx.setup_1d(p, cfg)) == 0
        ctx.upload(x0)
        ctx.run_range([3, 4, 5])
        got = ctx.download()
        assert int(ctx.stats().term_updates) == 3 * quota
    finally:
        ctx.close()
    assert not np.array_equal(bits(want), bits(x0))
    _same(cl, got, want, f"{cid} control, rank {rank}'s shard", "abi")


def test_rank_run_with_a_collective_of_three_threads():
    """gfs_rank_run itself, the way a host with one thread per GPU drives it: its own windows of 4 iterations, the
    collective a host-staged sum in rank order behind a barrier.  A failure on one thread aborts the barrier, so the
    others end instead of waiting."""
    case = MC.RUN_CASE
    cl = MC.restated(case.id)
    W = case.world
    rt = _rt()
    ranks = _ranks(case, cl)
    barrier = threading.Barrier(W, timeout=60)
    stage, sums, calls, errors, results = {}, {}, [[] for _ in range(W)], [None] * W, [None] * W

    def collective(rank):
        def allreduce(ptr, count, is_f64, stream):
            try:
                n = len(calls[rank])
                calls[rank].append((int(count), bool(is_f64)))
                assert rt.hipStreamSynchronize(C.c_void_p(stream or 0)) == 0
                host = _download(ptr, count, np.float64 if is_f64 else np.float32)
                stage[(n, rank)] = host
                barrier.wait()
                s = stage[(n, 0)].copy()
                for r in range(1, W):
                    s = s + stage[(n, r)]
                assert s.dtype == host.dtype
                if rank == 0:
                    sums[n] = s
                _upload(ptr, s)
            except BaseException as e:
                errors[rank] = e
                raise
        return allreduce

    def body(rank):
        try:
            ranks[rank].run(collective(rank))
            results[rank] = ranks[rank].get_positions()
        except BaseException as e:
            errors[rank] = errors[rank] or e
            barrier.abort()

    try:
        for x in MC.starts(case):
            for rk in ranks:
                rk.set_positions(x)
        threads = [threading.Thread(target=body, args=(r,)) for r in range(W)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads)
        assert errors == [None] * W, errors
        n_windows = len(cl.windows)
        assert [w["ks"] for w in cl.windows] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
        want_calls = [(2 * cl.total, False)] * n_windows + [(cl.g.n_nodes * cl.width, True)]
        assert calls == [want_calls] * W
        for i in range(n_windows):
            _same(cl, sums[i], cl.windows[i]["sum"], f"{case.id} collective {i}, the summed buffer", "exchange")
        _same(cl, sums[n_windows], cl.finishes[0]["x"][cl.abi_of_device], f"{case.id} final collective", "device")
        for r in range(W):
            _same(cl, results[r], cl.finishes[0]["x"], f"{case.id} rank {r}, final positions", "abi")
        assert [int(rk.info().windows) for rk in ranks] == [n_windows] * W
    finally:
        _close(ranks)
