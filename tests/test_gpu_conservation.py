"""Every full-width SGD kernel held to conservation and untouched sentinels (conservation.py): at 2048 streams — 32 waves on
the work pools, an odd number of updates per iteration so that every counter's last chunk is ragged — each counted update must
have delivered its two equal and opposite adds to the right two words.  A +r lost or doubled at a chunk seam, an add under a
wrong exec mask, an add to slot +-1 or with a wrong plane stride changes no count and heals inside every statistical margin;
here it moves the sum of a component or the bits of a sentinel.  The oracle's own drift under the same check and the proof that
the special trip forms are taken on this graph are in test_conservation_host.py."""
import numpy as np
import pytest

from util import G, P, gaussian_init
from quality_restatement import noisy_start
from conservation import guarded_graph, check, no_repeat_inside_a_path
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

UPDATES = 100003                      # odd: shares differ by one, last chunks are ragged
STREAMS = 2048
B64 = hip.F_BUNDLE(64)


@pytest.fixture(scope="module")
def guarded():
    """(g, node_perm, starts): the starts by dims (0: the sort), computed once and read-only."""
    g, perm = guarded_graph()
    starts = {0: noisy_start(g, 0, 7)}
    for dims in (2, 3, 4, 5, 8):
        starts[dims] = gaussian_init(g, dims, 7)
    for x in starts.values():
        x.setflags(write=False)
    return g, perm, starts


def _params(g, dims, iter_max=10):
    p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = iter_max
    return p


FUSED, UNFUSED = 1, 5                 # launches of one run_range over five iterations

CASES = [
    # id, dims (0: the sort), flags, n_streams, bundle, launches per range of five, phase window
    # 1D reference streams (K1d fused, K1 per iteration)
    ("1d-ref", 0, hip.F_BUNDLE(1), STREAMS, 1, FUSED, None),
    ("1d-ref-unfused", 0, hip.F_BUNDLE(1) | hip.F_NO_FUSE, STREAMS, 1, UNFUSED, None),
    ("1d-ref-2000-streams", 0, hip.F_BUNDLE(1), 2000, 1, FUSED, None),
    # 1D team kernels (K1b per iteration, K1c fused)
    ("1d-B4-unfused", 0, hip.F_BUNDLE(4) | hip.F_NO_FUSE, STREAMS, 4, UNFUSED, None),
    ("1d-B16", 0, hip.F_BUNDLE(16), STREAMS, 16, FUSED, None),
    ("1d-B64", 0, B64, STREAMS, 64, FUSED, None),
    ("1d-B64-one-partner", 0, B64 | hip.F_ONE_PARTNER, STREAMS, 64, FUSED, None),
    ("1d-B64-no-twin-trip", 0, B64 | hip.F_DBG_NO_TWIN_TRIP, STREAMS, 64, FUSED, None),
    ("1d-B64-no-fused-trip", 0, B64 | hip.F_DBG_NO_FUSED_TRIP, STREAMS, 64, FUSED, None),
    ("1d-B64-unfused", 0, B64 | hip.F_NO_FUSE, STREAMS, 64, UNFUSED, None),
    ("1d-B64-free-running", 0, B64 | hip.F_DBG_FREE_RUNNING, STREAMS, 64, FUSED, None),
    ("1d-B64-no-lds-tables", 0, B64 | hip.F_NO_LDS_TABLES, STREAMS, 64, FUSED, None),
    ("1d-B64-plain-loads", 0, B64 | hip.F_PLAIN_LOADS, STREAMS, 64, UNFUSED, None),          # plain loads do not fuse
    ("1d-B64-chain-1", 0, B64 | hip.F_CHAIN(1), STREAMS, 64, FUSED, None),
    ("1d-B64-wide-index", 0, B64 | hip.F_DBG_WIDE_INDEX, STREAMS, 64, FUSED, None),
    # phased (K1e): reference streams in iterations 2 and 3
    ("1d-phased", 0, hip.F_PHASED | B64, STREAMS, 64, FUSED, (2, 4)),
    # layout team kernels (K2b per iteration, K2c fused: B = 64 only)
    ("D2-B64", 2, B64, STREAMS, 64, FUSED, None),
    ("D2-B64-unfused", 2, B64 | hip.F_NO_FUSE, STREAMS, 64, UNFUSED, None),
    ("D2-B64-one-partner", 2, B64 | hip.F_ONE_PARTNER, STREAMS, 64, FUSED, None),
    ("D3-B64", 3, B64, STREAMS, 64, FUSED, None),
    ("D3-B64-unfused", 3, B64 | hip.F_NO_FUSE, STREAMS, 64, UNFUSED, None),
    ("D3-B64-one-partner", 3, B64 | hip.F_ONE_PARTNER, STREAMS, 64, FUSED, None),
    ("D2-B8", 2, hip.F_BUNDLE(8), STREAMS, 8, UNFUSED, None),                                # no fused kernel below B = 64
    ("D4-B64", 4, B64, STREAMS, 64, FUSED, None),
    ("D8-B64", 8, B64, STREAMS, 64, FUSED, None),
    ("D5-B16", 5, hip.F_BUNDLE(16), STREAMS, 16, UNFUSED, None),
    ("D2-B64-wide-index", 2, B64 | hip.F_DBG_WIDE_INDEX, STREAMS, 64, FUSED, None),
    # layout reference streams (K2d), here with sentinels and a permuted node layout
    ("D2-ref", 2, hip.F_BUNDLE(1), STREAMS, 1, FUSED, None),
    ("D8-ref", 8, hip.F_BUNDLE(1), STREAMS, 1, FUSED, None),
]


@pytest.mark.parametrize("name,dims,flags,n_streams,bundle,launches,window", CASES, ids=[c[0] for c in CASES])
def test_full_width_run_conserves_component_sums_and_leaves_sentinels(guarded, name, dims, flags, n_streams, bundle, launches, window):
    """Five iterations in one run_range, checked; five more on the same context (TeamState and the generators carry over),
    checked against the ORIGINAL start with the count of all ten."""
    g, perm, starts = guarded
    before = starts[dims]
    ctx = hip.Context(g, node_perm=perm)
    try:
        cfg = hip.make_config(n_streams=n_streams, term_updates_per_iteration=UPDATES, flags=flags)
        rc = ctx.setup_nd(_params(g, dims), cfg) if dims else ctx.setup_1d(_params(g, 0), cfg)
        assert rc == hip.OK
        assert np.array_equal(ctx.node_layout(), perm)
        if window is not None:
            assert ctx.phase_window(*window) == window
        ctx.upload(before)
        st0 = ctx.stats()
        assert (st0.n_streams, st0.bundle, st0.term_updates) == (n_streams, bundle, 0)
        for done, ks in ((5, range(5)), (10, range(5, 10))):
            ctx.run_range(list(ks))
            ctx.synchronize()
            st = ctx.stats()
            assert (st.n_streams, st.bundle) == (n_streams, bundle)
            assert st.launches - st0.launches == launches * done // 5, (st.launches, launches)
            assert st.term_updates == done * UPDATES
            check(before, ctx.download(), g, dims, st.term_updates, case=f"{name}-after-{done}")
    finally:
        ctx.close()


# ---- batches (K1f, K2f): reference streams of many contexts in one launch -------------------------------------------------
@pytest.mark.parametrize("dims", [0, 2], ids=["1d", "D2"])
def test_batch_items_conserve_and_a_bystander_is_untouched(guarded, dims):
    """Three items on guarded_graph(): the library's own stream count (several workgroups), 1000 streams (a ragged wave) and one
    stream, the first on the permuted node layout.  A fourth context, set up and loaded but not in the batch, keeps its bits."""
    g, perm, starts = guarded
    before = starts[dims]
    p = _params(g, dims, iter_max=4)
    ctxs = []
    try:
        for n_streams, node_perm in ((0, perm), (1000, None), (1, None), (0, perm)):
            ctx = hip.Context(g, node_perm=node_perm)
            ctxs.append(ctx)
            cfg = hip.make_config(n_streams=n_streams, term_updates_per_iteration=UPDATES)
            assert (ctx.setup_nd(p, cfg) if dims else ctx.setup_1d(p, cfg)) == hip.OK
            ctx.upload(before)
        items, bystander = ctxs[:3], ctxs[3]
        assert items[0].stats().n_streams > 2 * 256 and items[0].stats().bundle == 1
        b = hip.Batch(items)
        try:
            assert b.run() == hip.OK
            bs = b.stats()
            assert (bs.items, bs.items_run, bs.launches) == (3, 3, 1)
            assert bs.term_updates == 3 * 5 * UPDATES
        finally:
            b.close()
        for ctx, want_streams in zip(items, (items[0].stats().n_streams, 1000, 1)):
            st = ctx.stats()
            assert (st.n_streams, st.bundle, st.launches, st.iterations) == (want_streams, 1, 1, 5)
            assert st.term_updates == 5 * UPDATES
            check(before, ctx.download(), g, dims, st.term_updates, case=f"batch-{'D%d' % dims if dims else '1d'}-{want_streams}-streams")
        assert bystander.stats().term_updates == 0
        assert np.array_equal(bystander.download().view(np.uint64), before.view(np.uint64))
    finally:
        for ctx in ctxs:
            ctx.close()


# ---- the product's own policy: what the benchmark and the CLI run ----------------------------------------------------------
@pytest.fixture(scope="module")
def bubbles():
    g = G.synth_bubbles(20_000, 16, 5)
    assert g.n_nodes == 26250 and no_repeat_inside_a_path(g)
    return g


@pytest.mark.parametrize("dims", [0, 2, 3], ids=["sort", "D2", "D3"])
def test_default_policy_conserves_on_the_bubble_graph(bubbles, dims):
    """Default flags, default streams, the library's node layout: the team kernels at B = 64.  The graph
    is one component without sentinels: conservation only."""
    g = bubbles
    p = _params(g, dims, iter_max=4)
    before = gaussian_init(g, dims, 7) if dims else hip.init_positions(g)
    if dims:
        rc, after, st = hip.path_linear_sgd_layout_raw(g, p, before)
    else:
        rc, after, st = hip.path_linear_sgd_raw(g, p, x=before.copy())
    assert rc == hip.OK and st.bundle == 64
    assert st.term_updates == 5 * p.min_term_updates
    check(before, after, g, dims, st.term_updates, case=f"policy-{'D%d' % dims if dims else 'sort'}")
