"""The work-pool walk of the fused launches (sgd_kernel_common.h pool_walk) where single-wave tests cannot see it: 32 waves on two
counters, an odd number of updates per iteration — the counters' shares differ by one and neither is a multiple of a chunk, so
the last chunk of every counter is ragged — in ONE launch of five iterations.  Every iteration must apply exactly its updates,
whichever family of kernels walks the pool.  The contract of the launch, not of one implementation of the walk."""
import numpy as np
import pytest

from util import P, graph_from_paths, gaussian_init
from gfasort_amd import hip

pytestmark = pytest.mark.gpu

UPDATES = 100003                      # odd: two counters take 50002 and 50001
ITERATIONS = 5


def _graph():
    """A chain of 6000 nodes: one path over all of it and five over overlapping stretches of 1500 to 3000 steps."""
    rng = np.random.default_rng(11)
    n = 6000
    paths = [list(range(n))] + [list(range(s, s + w)) for s, w in ((0, 3000), (1000, 2500), (2500, 3000), (4000, 1500), (300, 2000))]
    return graph_from_paths(paths, rng.integers(1, 17, n))


@pytest.fixture(scope="module")
def graph():
    return _graph()


CASES = [
    # id, dims (0: the sort), flags, n_streams, phase window
    ("K1c", 0, hip.F_BUNDLE(64), 2048, None),
    ("K1d", 0, hip.F_BUNDLE(1), 2048, None),
    ("K1d-16-live-lanes", 0, hip.F_BUNDLE(1), 2000, None),
    ("K1e", 0, hip.F_PHASED | hip.F_BUNDLE(64), 2048, (2, 4)),          # reference streams in iterations 2 and 3
    ("K2c-D2", 2, hip.F_BUNDLE(64), 2048, None),
    ("K2c-D4-one-counter", 4, hip.F_BUNDLE(64), 2048, None),
    ("K2d-D2", 2, hip.F_BUNDLE(1), 2048, None),
]


@pytest.mark.parametrize("name,dims,flags,n_streams,window", CASES, ids=[c[0] for c in CASES])
def test_five_iterations_in_one_launch_apply_exactly_their_updates(graph, name, dims, flags, n_streams, window):
    g = graph
    cfg = hip.make_config(n_streams=n_streams, term_updates_per_iteration=UPDATES, flags=flags)
    ctx = hip.Context(g)
    try:
        if dims == 0:
            p = P.YgsParams.from_graph(g, 0, 1).path_sgd
            p.iter_max = 10
            ctx.setup_1d(p, cfg)
            x0 = hip.init_positions(g)
        else:
            p = P.LayoutSGDParams.from_graph(g, dims, 1)
            p.iter_max = 10
            ctx.setup_nd(p, cfg)
            x0 = gaussian_init(g, dims, 7)
        if window is not None:
            assert ctx.phase_window(*window) == window
        st0 = ctx.stats()
        assert st0.n_streams == n_streams and st0.bundle == (flags >> 16) & 0xFF
        for rerun in (False, True):                                           # the same configuration once more after reset_streams
            if rerun:
                ctx.reset_streams()
            ctx.upload(x0)
            before = ctx.stats()
            ctx.run_range(list(range(ITERATIONS)))
            ctx.synchronize()
            st = ctx.stats()
            assert st.launches - before.launches == 1
            assert st.term_updates - before.term_updates == ITERATIONS * UPDATES
            assert np.isfinite(ctx.download()).all()
    finally:
        ctx.close()
