"""The batched sort quality (K7k, batch_sort_quality_kernels.hip): gfs_batch_sort_quality gives, for every item of a batch of 1D
sorts in a number of launches that does not depend on the number of items, what gfs_ctx_sort_quality gives one item at a time —
field for field, sq_err_sum as bits — and touches nothing.

The batch (tests/batch_sort_quality_cases.py; tests/test_batch_sort_quality_host.py holds the generators to these facts): simple and
lil; DRB1 (4 955 nodes: P = 8192, the 96 KiB launch; 18 workgroups of the step pass); chains of 64 nodes (P = 64, one wave, no
LDS stage), 65 nodes (P = 128, the first LDS stage), 1 025 nodes (block 1024, two chunks of the scan) and 2 049 steps (two
workgroups); a one-node graph; a graph with a path but fewer than two steps; absent_node; and medium, just past 256 * 2048 steps
(257 workgroups: the reduce stages a second tile of partials) and above the sort cap (K6's path), last in the batch.

Positions: the K4b start; after a run() of the batch; uploaded positions with ties, NaN, both zeros and both infinities in DRB1 and
in the chain of 65 nodes (ties are broken by dense index, NaNs sort last).

Everything is compared exactly: there is no tolerance."""
import re
import struct

import numpy as np
import pytest

from util import P, load, cli_solo_and_batch
from gfasort_amd import build, hip
from quality_restatement import np_sort_quality, sort_step_values, tree_sum, noisy_start
import batch_sort_quality_cases as K

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = -1, -5
SUMS = ("steps", "abs_err_sum", "genomic_sum", "sq_err_sum")
ZERO_ROW = dict(steps=0, abs_err_sum=0, genomic_sum=0, sq_err_sum=0.0, mse=0.0, rmse=0.0, mae=0.0, relative_error=0.0)
STATES = ("start", "run", "special")


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _params(g, i, dims=0):
    p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.space = min(p.space, 20_000)                                       # (the zeta table has `space` entries: medium's is its longest path)
    p.min_term_updates = min(p.min_term_updates, 20_000)                 # a few short iterations: the run is here to move the positions
    p.iter_max = 2
    p.seed = 9399220 + i
    return p


def _batch(gs, n_streams=64, dims=0):
    """Set-up contexts (reference streams, so that graphs of 16 384 nodes and more may join) and their batch."""
    ctxs = []
    for i, g in enumerate(gs):
        ctx = hip.Context(g)
        rc = (ctx.setup_nd if dims else ctx.setup_1d)(_params(g, i, dims), hip.make_config(n_streams=n_streams, flags=hip.F_BUNDLE(1)))
        assert rc >= hip.OK                                              # (a graph without a path of two steps: nothing to do)
        ctxs.append(ctx)
    return ctxs, hip.Batch(ctxs)


def special_positions(g, seed):
    """Multiples of 8 bp (many ties), then NaNs, both zeros and both infinities sprinkled in."""
    rng = np.random.default_rng(seed)
    x = np.round(noisy_start(g, 0, seed, scale=40.0) / 8.0) * 8.0
    n = g.n_nodes
    for value, k in ((np.nan, 5), (-0.0, 7), (0.0, 7), (np.inf, 3), (-np.inf, 3), (-np.nan, 2)):
        x[rng.integers(0, n, k)] = value
    return x


def _set_state(state, gs, ctxs, b):
    if state == "start":
        b.init_positions()
    elif state == "run":
        b.init_positions()
        b.run()
    else:
        for i, (g, c) in enumerate(zip(gs, ctxs)):
            c.upload(special_positions(g, 50 + i) if K.NAMES[i] in ("DRB1", "chain65") else noisy_start(g, 0, 31 + i))


@pytest.fixture(scope="module", params=STATES)
def resident(request):
    """(state, graphs, contexts, batch, the batch's rows at the default cap), built once per state and only read."""
    gs = K.graphs()
    ctxs, b = _batch(gs)
    _set_state(request.param, gs, ctxs, b)
    rows, ms = b.sort_quality(return_kernel_ms=True)
    assert ms > 0.0 and len(rows) == len(gs)
    yield request.param, gs, ctxs, b, rows
    b.close()
    for c in ctxs:
        c.close()


def raw_rows(b):
    """The call's own bytes: n rows of gfs_sort_quality."""
    out = np.zeros(len(b.contexts), dtype=hip.SORT_QUALITY_DTYPE)
    assert hip.lib().gfs_batch_sort_quality(b._h, hip._ptr(out), len(b.contexts), None, None) == hip.OK, hip.lib().gfs_last_error()
    return out.tobytes()


# ---- 1: the item's own call ---------------------------------------------------------------------------------------------------------
def test_rows_are_the_contexts_own_field_for_field(resident):
    state, gs, ctxs, b, rows = resident
    for i, c in enumerate(ctxs):
        try:
            own = c.sort_quality()
        except hip.GfsError:
            own = ZERO_ROW                                               # where the item's own call refuses, the row is zeros
        print(state, K.NAMES[i], {k: rows[i][k] for k in SUMS}, "rmse", rows[i]["rmse"])
        assert rows[i].keys() == own.keys()
        for k in own:
            assert bits(rows[i][k]) == bits(own[k]) if isinstance(own[k], float) else rows[i][k] == own[k], (state, K.NAMES[i], k)
    assert rows[K.NAMES.index("one_step")] == ZERO_ROW
    assert rows[K.NAMES.index("one_node")]["steps"] == 2 and rows[K.NAMES.index("medium")]["steps"] > 500_000


# ---- 2: the restatements ------------------------------------------------------------------------------------------------------------
def test_rows_are_the_restatements(resident):
    state, gs, ctxs, b, rows = resident
    _, orders, _ = b.results(positions=False)
    for i, (g, c) in enumerate(zip(gs, ctxs)):
        order = orders[i]
        if state == "special" and K.NAMES[i] in ("DRB1", "chain65"):
            x = c.download()
            key = np.where(np.isnan(x), np.inf, x + 0.0)                 # ties by dense index; NaNs last, behind +inf
            want_order = np.lexsort((np.arange(g.n_nodes), np.isnan(x), key))
            assert np.array_equal(order, want_order.astype(np.uint64)), K.NAMES[i]
            assert np.isnan(x).sum() >= 2 and np.isinf(x).sum() >= 2 and np.unique(x[np.isfinite(x)]).shape[0] < g.n_nodes
        if g.n_steps < 2:
            assert rows[i] == ZERO_ROW
            continue
        want = np_sort_quality(g, order)
        for k in ("steps", "abs_err_sum", "genomic_sum"):
            assert rows[i][k] == want[k], (state, K.NAMES[i], k)
        ae, counted = sort_step_values(g, order)
        sq = ae.astype(np.float64) * ae.astype(np.float64)
        assert bits(rows[i]["sq_err_sum"]) == bits(tree_sum(sq, counted, g.n_steps)), (state, K.NAMES[i])


# ---- 3: the sort cap, and a second call ---------------------------------------------------------------------------------------------
def test_every_byte_is_independent_of_the_sort_cap_and_repeatable(resident):
    state, gs, ctxs, b, rows = resident
    want = raw_rows(b)
    assert raw_rows(b) == want                                           # a second call, the same bytes
    try:
        for cap in (64, 128, 0):                                         # items move between the LDS path and K6's
            b.debug_sort_cap(cap)
            assert raw_rows(b) == want, (state, cap)
    finally:
        b.debug_sort_cap(0)
    again = b.sort_quality()
    assert again == rows


# ---- 4: nothing but the output is written -------------------------------------------------------------------------------------------
def test_a_read_out_between_two_runs_leaves_the_second_run_alone():
    """Positions, counters and a following run() with the read-out in between are those without it."""
    gs = [K.chain(2049, 2), load("lil.gfa"), load("simple.gfa")]
    ctxs, b = _batch(gs, n_streams=1)                                    # one stream: a run is a function of its start
    plain, pb = _batch(gs, n_streams=1)
    counters = lambda c: (c.stats().term_updates, c.stats().attempts, c.stats().iterations, c.stats().launches)
    for bb in (b, pb):
        bb.init_positions()
        bb.run()
    before = [(c.download(), counters(c)) for c in ctxs]
    first = b.sort_quality()
    try:
        for cap in (64, 0):
            b.debug_sort_cap(cap)
            assert b.sort_quality() == first
    finally:
        b.debug_sort_cap(0)
    for c, (x, st) in zip(ctxs, before):
        assert np.array_equal(c.download().view(np.uint64), x.view(np.uint64)) and counters(c) == st
    b.run()
    pb.run()
    for c, q in zip(ctxs, plain):
        assert np.array_equal(c.download().view(np.uint64), q.download().view(np.uint64)) and counters(c) == counters(q)
        assert counters(c)[2:] == (6, 2)
    assert b.sort_quality() == pb.sort_quality()
    b.close()
    pb.close()
    for c in ctxs + plain:
        c.close()


# ---- 5: refusals, each before any write ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched():
    gs = [load("lil.gfa"), load("simple.gfa")]
    L, p = hip.lib(), hip._ptr
    out = np.zeros(3, dtype=hip.SORT_QUALITY_DTYPE)
    out[:] = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 7, -1.5)
    sentinel = out.tobytes()
    ctxs, b = _batch(gs)
    for n in (1, 3, 0):
        assert L.gfs_batch_sort_quality(b._h, p(out), n, None, None) == E_ARG and b"item count" in L.gfs_last_error()
    assert L.gfs_batch_sort_quality(b._h, None, 2, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert L.gfs_batch_sort_quality(None, p(out), 2, None, None) == E_ARG and b"null" in L.gfs_last_error()
    assert out.tobytes() == sentinel
    lctxs, lb = _batch(gs, dims=2)
    assert L.gfs_batch_sort_quality(lb._h, p(out), 2, None, None) == E_UNSUPPORTED and b"a batch of layouts" in L.gfs_last_error()
    with pytest.raises(hip.GfsError) as e:
        lb.sort_quality()
    assert e.value.code == E_UNSUPPORTED
    assert out.tobytes() == sentinel
    for h in (b, lb):
        h.close()
    for c in ctxs + lctxs:
        c.close()


# ---- 6: the one-shot entry ------------------------------------------------------------------------------------------------------------
def test_the_one_shot_entry_equals_the_resident_call(resident):
    state, gs, ctxs, b, rows = resident
    for name in ("lil", "DRB1", "chain65", "absent_node", "one_step"):
        i = K.NAMES.index(name)
        got = hip.sort_quality(gs[i], ctxs[i].download())
        assert got.keys() == rows[i].keys()
        for k in got:
            assert bits(got[k]) == bits(rows[i][k]) if isinstance(got[k], float) else got[k] == rows[i][k], (state, name, k)


# ---- 7: the command line --------------------------------------------------------------------------------------------------------------
FIXTURES = ["simple.gfa", "lil.gfa", "DRB1-3123.gfa"]
LINE = re.compile(r"^\[gfasort\] sort quality: steps=\d+ abs_err_sum=\d+ genomic_sum=\d+ rmse_bp=\S+ mae_bp=\S+ relative_error=\S+$", re.M)


def test_cli_batch_sort_quality_prints_what_the_single_runs_print(tmp_path):
    build.build_host()
    flags = ["-p", "Y", "--streams", "1", "-v", "1", "--iter-max", "2", "--sort-quality"]
    solo, r = cli_solo_and_batch(build.CLI, tmp_path, FIXTURES, flags, layouts=False)
    assert all(s.returncode == 0 for s in solo), [s.stderr for s in solo]
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("in the batch") == len(FIXTURES), r.stderr
    want = [line for s in solo for line in LINE.findall(s.stderr)]
    got = LINE.findall(r.stderr)
    print("\n".join(got))
    assert len(want) == len(FIXTURES) and got == want
    assert all(s.stderr.count("sort quality:") == 1 for s in solo) and r.stderr.count("sort quality:") == len(FIXTURES)
    quiet = cli_solo_and_batch(build.CLI, tmp_path, FIXTURES[:1], [f for f in flags if f != "--sort-quality"], layouts=False)[1]
    assert quiet.returncode == 0 and "sort quality" not in quiet.stderr
    import subprocess
    refused = subprocess.run([build.CLI, "-i", "in.gfa", "-o", "out.gfa", "-p", "L", "--sort-quality"], capture_output=True, text=True)
    assert refused.returncode == 2 and "--sort-quality" in refused.stderr and "no Y step" in refused.stderr
