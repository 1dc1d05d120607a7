"""The one-off position passes of a single context (csrc/index_kernels.hip), each against a plain restatement
(tests/position_passes_ref.py), bit for bit, past the grid seam of its kernels and under a caller's layout that is neither the
identity nor path order:

  reorder_positions_kernel   upload and download, read and written in device memory directly (tests/device_raw.py), each
                             direction on its own: D = 0 (1D) and every D = 1..8
  K4                         gfs_ctx_init_positions against the integer prefix sum, totals past 2^32 and past 2^53 included
  K6                         gfs_ctx_sort_order against a lexsort, on NaNs, zeros, infinities, denormals and ties

Every other test passes its data through these three, so a fault here corrupts everything silently; a round trip
download(upload(x)) == x passes for any mapping that is wrong consistently, which is why the device vector itself is read.
Every comparison is on bit patterns; there is no tolerance in this file."""
import functools

import numpy as np
import pytest

import position_passes_ref as R
from device_raw import Dev, download as raw_download, upload as raw_upload
from gfasort_amd import hip, params as P
from gfasort_amd.distributed import path_order_layout

pytestmark = pytest.mark.gpu

CFG = dict(n_streams=64, flags=hip.F_BUNDLE(1))     # (nothing runs: the set-up is here for the position vector it allocates)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _graph(n):
    """A chain of n nodes under two paths, lengths 1..16; only read."""
    return R.chain_under_two_paths(n, np.random.default_rng(n).integers(1, 17, n))


@functools.lru_cache(maxsize=None)
def _layout(n):
    """The caller's layout of _graph(n): a seeded random permutation, not the identity, not path order; only read."""
    own = path_order_layout(_graph(n))
    perm = R.random_layout(n, 1000 + n, avoid=(own,))
    if n >= 3:
        assert not np.array_equal(perm, np.arange(n)) and not np.array_equal(perm, own)
    perm.setflags(write=False)
    return perm


def _context(g, dims, perm):
    """A context of g under the layout `perm` (None: the library's own), set up for `dims` (0: the 1D sort).  Returns (ctx, perm)."""
    ctx = hip.Context(g, node_perm=perm)
    try:
        if dims:
            rc = ctx.setup_nd(P.LayoutSGDParams(dimensions=dims, iter_max=2, min_term_updates=1000), hip.make_config(**CFG))
        else:
            rc = ctx.setup_1d(P.PathSGDParams(iter_max=2, min_term_updates=1000), hip.make_config(**CFG))
        assert rc == (hip.OK if g.path_step_counts().max() > 1 else hip.NOTHING_TO_DO)
        assert ctx.positions_len() == g.n_nodes * (2 * dims if dims else 1)
        layout = ctx.node_layout()
        if perm is not None:
            assert np.array_equal(layout, perm)
        else:
            assert np.array_equal(layout, path_order_layout(g))
        return ctx, layout
    except BaseException:
        ctx.close()
        raise


def _device_vector(ctx):
    return raw_download(ctx.positions_device(), ctx.positions_len(), np.float64)


def _same(got, want, space, n, dims, where, marked=True):
    text = R.first_difference(got, want, space, n, dims, marked)
    if text:
        pytest.fail(where + ": " + text)


def _sizes(dims):
    return R.EDGE_SIZES + (R.SEAM,) + ((R.SEAM_1D_COPY,) if dims == 0 else ())


# ---- 1. the device order, read directly ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", range(9))
def test_upload_puts_every_element_where_the_device_order_says(dims):
    """gfs_ctx_upload_positions, then the device vector as it lies in memory: dev[(end*D + dim)*N + perm[k]] is the element
    (k, end, dim) of what was uploaded.  At the seam size the copy's grid-stride loop takes a second pass (N * 2D > 524 288)."""
    for n in _sizes(dims):
        ctx, perm = _context(_graph(n), dims, _layout(n))
        try:
            v = R.abi_pattern(n, dims, tag=1)
            ctx.upload(v)
            _same(_device_vector(ctx), R.to_device(v, perm, dims), "device", n, dims, "after upload")
        finally:
            ctx.close()


@pytest.mark.parametrize("dims", range(9))
def test_download_reads_every_element_from_where_the_device_order_says(dims):
    """A device-order vector written straight into the context's buffer, then gfs_ctx_download_positions: element (k, end, dim)
    is dev[(end*D + dim)*N + perm[k]].  Nothing is uploaded through the library: this does not rest on the test above."""
    for n in _sizes(dims):
        ctx, perm = _context(_graph(n), dims, _layout(n))
        try:
            dev = R.device_pattern(n, dims, tag=2)
            raw_upload(ctx.positions_device(), dev)
            _same(ctx.download(), R.to_abi(dev, perm, dims), "abi", n, dims, "download")
            _same(_device_vector(ctx), dev, "device", n, dims, "the device vector after a download")     # (it only reads)
        finally:
            ctx.close()


@pytest.mark.parametrize("dims,n", [(0, R.SEAM_1D_COPY), (2, 257), (3, R.SEAM)])
def test_both_directions_under_the_librarys_own_layout(dims, n):
    ctx, perm = _context(_graph(n), dims, None)
    try:
        assert not np.array_equal(perm, np.arange(n))                    # (S lines are shuffled: path order is not dense order)
        v = R.abi_pattern(n, dims, tag=3)
        ctx.upload(v)
        _same(_device_vector(ctx), R.to_device(v, perm, dims), "device", n, dims, "after upload")
        dev = R.device_pattern(n, dims, tag=4)
        raw_upload(ctx.positions_device(), dev)
        _same(ctx.download(), R.to_abi(dev, perm, dims), "abi", n, dims, "download")
    finally:
        ctx.close()


@pytest.mark.parametrize("dims,n", [(0, 257), (3, R.SEAM)])
def test_both_directions_on_bound_positions_leave_the_words_around_them(dims, n):
    """gfs_ctx_bind_positions on a buffer of the test's own, one word longer at either end: both directions act on the bound
    buffer, and the two words around x_len come back untouched."""
    ctx, perm = _context(_graph(n), dims, _layout(n))
    x_len = ctx.positions_len()
    buf = Dev(x_len + 2, np.float64)
    try:
        guard = R.marks([7, 8], 1, 1, tag=200).view(np.float64)
        whole = np.concatenate([guard[:1], R.device_pattern(n, dims, tag=5), guard[1:]])
        buf.set(whole)
        ctx.bind_positions(buf.ptr + 8)
        assert ctx.positions_device() == buf.ptr + 8 and ctx.positions_len() == x_len
        v = R.abi_pattern(n, dims, tag=6)
        ctx.upload(v)
        got = buf.host()
        _same(got[1:-1], R.to_device(v, perm, dims), "device", n, dims, "bound buffer after upload")
        assert np.array_equal(_bits(got[[0, -1]]), _bits(guard)), "upload wrote outside the bound vector"
        dev = R.device_pattern(n, dims, tag=7)
        whole = np.concatenate([guard[:1], dev, guard[1:]])
        buf.set(whole)
        _same(ctx.download(), R.to_abi(dev, perm, dims), "abi", n, dims, "download from the bound buffer")
        assert np.array_equal(_bits(buf.host()), _bits(whole)), "download wrote to the bound buffer or around it"
    finally:
        ctx.close()
        buf.free()


# ---- 2. K4 against an integer prefix sum ----------------------------------------------------------------------------------------
def _k4(g, perm, raw=False, where=""):
    """gfs_ctx_init_positions of a context of g under `perm`, and the host's gfs_init_positions, each against the integer sum."""
    n = g.n_nodes
    want = R.prefix_positions(g.node_len)
    _same(hip.init_positions(g), want, "abi", n, 0, where + " host gfs_init_positions", marked=False)
    ctx, layout = _context(g, 0, perm)
    try:
        _k4_on(ctx, layout, want, raw, where)
    finally:
        ctx.close()
    return want


def _k4_on(ctx, layout, want, raw, where):
    n = want.shape[0]
    raw_upload(ctx.positions_device(), R.device_pattern(n, 0, tag=8))     # a word K4 skips keeps its mark (a zero would hide it)
    ctx.init_positions()
    if raw:
        _same(_device_vector(ctx), R.to_device(want, layout, 0), "device", n, 0, where + " K4, device vector", marked=False)
    _same(ctx.download(), want, "abi", n, 0, where + " K4 through download", marked=False)


@pytest.mark.parametrize("n", R.EDGE_SIZES)
def test_k4_at_the_edge_sizes(n):
    g = R.chain_under_two_paths(n, R.mixed_lengths(n, n) if n > 2 else np.full(n, 5))
    _k4(g, R.random_layout(n, 50 + n), raw=True, where=f"N = {n}")
    _k4(g, None, where=f"N = {n}, own layout")


def test_k4_past_the_seam_with_zero_length_nodes():
    lens = R.mixed_lengths(R.SEAM, 21)
    assert lens[0] == 0 and lens[-1] == 0 and ((lens[1:] == 0) & (lens[:-1] == 0)).sum() > 100
    want = _k4(R.chain_under_two_paths(R.SEAM, lens), _layout(R.SEAM), raw=True, where="mixed lengths")
    assert (np.diff(want) == 0).sum() > 30_000                            # equal positions do occur


def test_k4_past_the_seam_under_the_librarys_own_layout():
    _k4(R.chain_under_two_paths(R.SEAM, R.mixed_lengths(R.SEAM, 22)), None, raw=True, where="own layout")


def test_k4_with_totals_past_2_32():
    lens = R.huge_lengths(R.SEAM, 23)
    sums = R.prefix_sums(lens)
    assert int(lens.max()) == 0xFFFFFFFF and int(sums[2]) > 1 << 32 and int(sums[-1]) > 1 << 49
    _k4(R.chain_under_two_paths(R.SEAM, lens), _layout(R.SEAM), raw=True, where="totals past 2^32")


def test_k4_with_totals_past_2_53():
    """2 500 000 nodes of 2^32 - 1 or 2^32 - 2 bp: from about node 2.1 M on the sums pass 2^53, where an odd sum is no double and
    the conversion rounds to nearest even.  Two paths of two steps each: no path comes near the 2^55 bp a step record holds."""
    n = 2_500_000
    rng = np.random.default_rng(24)
    lens = (0xFFFFFFFF - rng.integers(0, 2, n)).astype(np.uint32)
    sums = R.prefix_sums(lens)
    past = sums > np.uint64(1 << 53)
    assert past.sum() > 1000 and (sums[past] & np.uint64(1)).sum() > 100
    want = R.prefix_positions(lens)
    assert (want[past].astype(np.uint64) != sums[past]).sum() > 100      # the conversion does round
    g = R.chain_under_two_paths(n, lens, steps_per_path=2)
    assert g.path_step_counts().tolist() == [2, 2]
    _k4(g, R.random_layout(n, 25), where="totals past 2^53")


@pytest.mark.parametrize("n", [257, R.SEAM])
def test_k4_with_every_length_zero(n):
    want = _k4(R.chain_under_two_paths(n, np.zeros(n, np.uint32)), _layout(n), raw=True, where="all lengths 0")
    assert not _bits(want).any()                                         # +0.0, bit for bit


def test_k4_on_an_item_of_a_context_set():
    """An item's node lengths and layout are borrowed from the set's arena: the item gives the bits of its solo context."""
    n = 10_000
    g = R.chain_under_two_paths(n, R.huge_lengths(n, 26))
    assert int(R.prefix_sums(g.node_len)[2]) > 1 << 32
    want = R.prefix_positions(g.node_len)
    others = [_graph(257), R.chain_under_two_paths(65, np.zeros(65, np.uint32)), _graph(63)]
    graphs = others[:2] + [g] + others[2:]
    cs = hip.ContextSet(graphs)
    solo = None
    try:
        for i, (ctx, gi) in enumerate(zip(cs.contexts, graphs)):
            assert ctx.setup_1d(P.PathSGDParams(iter_max=2, min_term_updates=1000), hip.make_config(**CFG)) == hip.OK
            layout = ctx.node_layout()
            assert np.array_equal(layout, path_order_layout(gi))
            _k4_on(ctx, layout, R.prefix_positions(gi.node_len), True, f"set item {i}")
        solo, layout = _context(g, 0, None)
        _k4_on(solo, layout, want, True, "solo")
        _same(cs.contexts[2].download(), solo.download(), "abi", n, 0, "set item against its solo context", marked=False)
        _same(_device_vector(cs.contexts[2]), _device_vector(solo), "device", n, 0, "set item against its solo context", marked=False)
    finally:
        if solo is not None:
            solo.close()
        cs.close()


# ---- 3. K6 on hostile values under a foreign layout -----------------------------------------------------------------------------
def _same_order(got, want, x, where):
    got = np.asarray(got)
    assert got.dtype == np.uint64 and got.shape == want.shape, (where, got.dtype, got.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        r = int(bad[0])
        pytest.fail(f"{where}: {bad.size} of {want.shape[0]} ranks differ, the first is rank {r}: node {int(got[r])} "
                    f"(position {x[int(got[r]) % x.shape[0]]!r}) where node {int(want[r])} (position {x[int(want[r])]!r}) belongs")


@pytest.mark.parametrize("own_layout", [False, True], ids=["given-layout", "own-layout"])
def test_k6_on_hostile_values_past_the_seam(own_layout):
    n = R.SEAM
    x = R.hostile_positions(n, 31)
    b, nan = _bits(x), np.isnan(x)
    assert (nan & (b >> np.uint64(63) == 1)).sum() >= 2 and (nan & (b >> np.uint64(63) == 0)).sum() >= 2
    assert (x == np.inf).any() and (x == -np.inf).any()
    zeros = np.flatnonzero(x == 0.0)
    assert (b[zeros] == 0).any() and (b[zeros] != 0).any()               # both zeros: equal in value, adjacent in any order
    assert (np.diff(b[zeros].astype(np.int64) >> 63) != 0).sum() >= 8    # ... and they alternate in dense order
    assert np.unique(x[np.isfinite(x)]).shape[0] < n // 8                # fewer distinct finite values than nodes: ties
    want = R.sort_reference(x)
    assert np.array_equal(want[-nan.sum():], np.flatnonzero(nan).astype(np.uint64))   # NaNs last, in dense order
    _same_order(hip.sort_order(x), want, x, "host gfs_sort_order")
    ctx, _ = _context(_graph(n), 0, None if own_layout else _layout(n))
    try:
        ctx.upload(x)
        _same_order(ctx.sort_order(), want, x, "K6")
        _same(ctx.download(), x, "abi", n, 0, "positions after the sort", marked=False)      # the sort reads and does not write
    finally:
        ctx.close()


@pytest.mark.parametrize("n", R.EDGE_SIZES)
def test_k6_keeps_dense_order_where_every_position_is_equal(n):
    """The order is the identity although the layout is not: ties fall by dense index, not by slot."""
    x = np.full(n, 7.25)
    ctx, perm = _context(_graph(n), 0, _layout(n))
    try:
        assert n < 2 or not np.array_equal(perm, np.arange(n))
        ctx.upload(x)
        _same_order(ctx.sort_order(), np.arange(n, dtype=np.uint64), x, f"K6, N = {n}")
        _same_order(hip.sort_order(x), np.arange(n, dtype=np.uint64), x, f"host, N = {n}")
    finally:
        ctx.close()
