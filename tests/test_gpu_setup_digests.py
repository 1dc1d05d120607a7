"""gfs_ctx_setup_1d / _nd and gfs_ctx_reset_streams are a set setup and a seeding launch of one item (csrc/capi_set.hip
setup_contexts), so "an item equals the context set up alone" (tests/test_gpu_set_setup.py) compares one text with itself.  The
anchors here do not run the code under test: (1) the digests of every state array that scripts/setup_state_digest.py recorded at the
last commit whose single setup had a text of its own (tests/golden/setup_state_digests.json; the script's header names the commit),
and (2) the numpy restatement of the seeding and the host's own zeta table.  Integer arithmetic and host tables only: every
comparison is exact."""
import importlib.util
import json
import os

import numpy as np
import pytest

from util import GOLDEN, ROOT, load
from set_setup_ref import seeded_words
from test_gpu_set_setup import _base_1d, _with
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("setup_state_digest", os.path.join(ROOT, "scripts", "setup_state_digest.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

with open(os.path.join(GOLDEN, "setup_state_digests.json")) as f:
    RECORDED = json.load(f)


# ---- 1: against the recorded digests -------------------------------------------------------------------------------------------------
def test_the_recorded_cases_are_the_scripts():
    assert list(RECORDED) == list(D.CASES)


@pytest.mark.parametrize("name", list(D.CASES))
def test_state_digests_equal_the_recorded_ones(name):
    got = json.loads(json.dumps(D.CASES[name]()))                      # (tuples and None as the file has them)
    want = RECORDED[name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, k, {key: (g.get(key), w.get(key)) for key in w if g.get(key) != w.get(key)})


def test_the_refused_setup_keeps_a_zeroed_replica_and_nothing_else():
    """What the recorded case says, spelt out: the parent's error, a replica of n_nodes zeros, no streams, no state to reset."""
    (r,) = RECORDED["refused by the launch policy"]
    assert r["rc"] == -1 and "block_size must be a multiple of 64" in r["error"] and "set item" not in r["error"]
    assert r["positions_len"] == load("lil.gfa").n_nodes and r["has_positions"] and r["positions_zero"]
    assert r["n_streams"] == 0 and all(r[call][1].endswith("context not set up") for call in ("state", "reset", "run"))


def test_the_device_holds_the_callers_tables():
    p, cfg, tables = D.caller_tables()
    ctx = hip.Context(load("DRB1-3123.gfa"))
    try:
        for k, (etas, zetas) in enumerate(tables):
            assert ctx.setup_1d(p, cfg, etas=etas, zetas=zetas) == hip.OK
            assert ctx.debug_sgd_state(hip.STATE_ZETAS).tobytes() == zetas.tobytes(), k
            assert ctx.debug_sgd_state(hip.STATE_SCHEDULE)["eta"].tobytes() == etas.tobytes(), k
        assert not np.array_equal(tables[0][0], tables[1][0]) and not np.array_equal(tables[0][1], tables[2][1])
    finally:
        ctx.close()


# ---- 2: independent of any recorded file -------------------------------------------------------------------------------------------
def _chain_ctx():
    from test_gpu_set_setup import _chain
    return hip.Context(_chain(600, 5))


@pytest.mark.parametrize("seed, stream_base, T", [(11, 0, 1), (17, 0, 255), (29, (1 << 64) - 100, 256), (31, 7, 257), ((1 << 64) - 2, 0, 70)])
def test_rng_words_after_setup_and_after_reset_are_the_restatements(seed, stream_base, T):
    """Either side of the seeding kernel's workgroup of 256, one stream, and seed + t wrapping inside the context."""
    want = seeded_words(seed, stream_base, T)
    ctx = _chain_ctx()
    try:
        assert ctx.setup_1d(_with(_base_1d(iter_max=3, updates=500), seed=seed), hip.make_config(n_streams=T, stream_base=stream_base)) == hip.OK
        assert int(ctx.stats().n_streams) == T
        assert np.array_equal(ctx.debug_sgd_state(hip.STATE_RNG), want)
        ctx.init_positions()
        ctx.run_range([0, 1])
        ctx.synchronize()
        assert not np.array_equal(ctx.debug_sgd_state(hip.STATE_RNG), want)      # (the run advanced them)
        assert int(ctx.stats().term_updates) == 2 * 500
        ctx.reset_streams()
        assert np.array_equal(ctx.debug_sgd_state(hip.STATE_RNG), want)
        assert not ctx.debug_sgd_state(hip.STATE_COUNTERS).any() and int(ctx.stats().iterations) == 0
    finally:
        ctx.close()


def test_reset_streams_of_a_sets_item_reseeds_that_item_alone():
    """An item in the middle of a set's seeding launch (its first workgroup is not the launch's first) is reseeded by a launch of
    its own; its neighbours' words stay where their runs left them."""
    from test_gpu_set_setup import _chain
    graphs = [_chain(300, 2), _chain(400, 3), _chain(500, 4)]
    params = [_with(_base_1d(iter_max=3, updates=500), seed=40 + i) for i in range(3)]
    cfgs = [hip.make_config(n_streams=T) for T in (300, 257, 70)]
    cset = hip.ContextSet(graphs)
    try:
        assert cset.setup_1d(params, cfgs) == [hip.OK] * 3
        for c in cset.contexts:
            c.init_positions()
            c.run_range([0])
            c.synchronize()
        ran = [c.debug_sgd_state(hip.STATE_RNG) for c in cset.contexts]
        cset.contexts[1].reset_streams()
        assert np.array_equal(cset.contexts[1].debug_sgd_state(hip.STATE_RNG), seeded_words(41, 0, 257))
        assert not np.array_equal(ran[1], seeded_words(41, 0, 257))
        for i in (0, 2):
            assert np.array_equal(cset.contexts[i].debug_sgd_state(hip.STATE_RNG), ran[i]), i
    finally:
        cset.close()


@pytest.mark.parametrize("name, params_of", [("lil.gfa", "lil.gfa"), ("DRB1-3123.gfa", "lil.gfa"), ("lil.gfa", "DRB1-3123.gfa"),
                                             ("DRB1-3123.gfa", "DRB1-3123.gfa")])
def test_the_device_zeta_table_is_a_prefix_of_the_hosts_then_zeros(name, params_of):
    """DESIGN K3c point 3: the table a setup sums — to the clamped space — is a prefix of the table of the caller's space, bit for
    bit; everything behind the prefix is the zero padding up to the full length.  With the space of DRB1-3123 (its longest path
    in bp, past space_max: quantized entries) on the short paths of lil.gfa the clamp cuts most of the table."""
    from util import P
    g = load(name)
    p = P.YgsParams.from_graph(load(params_of), 0, 1).path_sgd
    p.iter_max, p.min_term_updates = 6, 2000
    full = hip.zeta_table(p)
    ctx = hip.Context(g)
    try:
        assert ctx.setup_1d(p, hip.make_config(n_streams=70)) == hip.OK
        z = ctx.debug_sgd_state(hip.STATE_ZETAS)
        assert len(z) == len(full)
        nz = np.flatnonzero(z)
        m = int(nz[-1]) + 1
        assert m >= 2 and z[0] == 0.0 and len(nz) == m - 1               # (entry 0 is zero in the host's table too; no hole behind it)
        print(f"{name} with the parameters of {params_of}: {m} of {len(full)} entries summed")
        assert z[:m].tobytes() == full[:m].tobytes()
        assert not z[m:].any()
        if (name, params_of) == ("lil.gfa", "DRB1-3123.gfa"):
            assert m < len(full)
    finally:
        ctx.close()
