"""conservation.py without a GPU: the oracle alone stays inside the bound on guarded_graph() in every mirror form the GPU cases
run, the graph reaches the special trip forms at their configuration, and the checker fails on corrupted output."""
import functools

import numpy as np
import pytest

from util import O, P, oracle_graph, oracle_params, gaussian_init
from quality_restatement import noisy_start
from conservation import guarded_graph, check, N_A, N_B, N_SENTINELS, NO_NODE

UPDATES = 100003
ITERATIONS = 10
STREAMS = 2048

# the product's defaults at B = 64 (GFS_F_CHAIN auto, two partners for the sort and layouts of 2 and 3 dimensions)
TEAM_1D = dict(bundle=64, partners=2, chain=64, twin_trip=True, fused_trip=True)
FORMS_1D = {
    "reference-streams": dict(bundle=1),
    "team": TEAM_1D,
    "team-one-partner": dict(TEAM_1D, partners=1),
    "team-chain-1": dict(TEAM_1D, chain=1),
    "team-no-twin-trip": dict(TEAM_1D, twin_trip=False),
    "team-no-fused-trip": dict(TEAM_1D, fused_trip=False),
}
FORMS_ND = {2: dict(bundle=64, partners=2, chain=16), 4: dict(bundle=64, partners=1, chain=16)}


@functools.lru_cache(maxsize=None)
def _graph():
    return guarded_graph()


def _params(g, dims):
    p = P.LayoutSGDParams.from_graph(g, dims, 1) if dims else P.YgsParams.from_graph(g, 0, 1).path_sgd
    p.iter_max = 10
    p.min_term_updates = UPDATES
    return p


def _start(g, dims):
    return gaussian_init(g, dims, 7) if dims else noisy_start(g, 0, 7)


def _oracle_run(dims, n_streams, **form):
    """(before, after, term_updates) of ITERATIONS oracle iterations on guarded_graph(), aligned to its node_perm."""
    g, perm = _graph()
    before = _start(g, dims)
    after = before.copy()
    st = O.State(oracle_graph(g), oracle_params(_params(g, dims)), dims=dims, n_streams=n_streams, node_slots=perm, **form)
    for k in range(ITERATIONS):
        st.run_iteration(k, after)
    updates = st.stats().term_updates
    st.close()
    assert updates == ITERATIONS * UPDATES
    return before, after, updates


@functools.lru_cache(maxsize=None)
def _oracle_1d_team():
    before, after, updates = _oracle_run(0, STREAMS, **TEAM_1D)
    before.setflags(write=False)
    after.setflags(write=False)
    return before, after, updates


def test_guarded_graph_is_what_the_cases_need():
    g, perm = _graph()
    assert g.n_nodes == N_A + N_B + N_SENTINELS == 8500 < 16384
    assert g.n_paths == 8 and int(g.path_step_counts().min()) >= 1024 and int((g.step_node == NO_NODE).sum()) == 12
    a, b, s = g.components["A"], g.components["B"], g.sentinels
    assert (a.shape[0], b.shape[0], s.shape[0]) == (N_A, N_B, N_SENTINELS)
    assert np.array_equal(np.sort(np.concatenate([a, b, s])), np.arange(g.n_nodes))
    first = g.path_first_step.astype(np.int64)
    in_a = np.isin(g.step_node, a)
    for pth in range(g.n_paths):                                               # a path stays inside one component
        seg = g.step_node[first[pth]:first[pth + 1]]
        part = in_a[first[pth]:first[pth + 1]][seg != NO_NODE]
        assert part.all() == (pth < 6) and part.any() == (pth < 6)
    kind = np.zeros(g.n_nodes, dtype=np.int8)                                  # interleaved: every part in every tenth of both orders
    kind[b], kind[s] = 1, 2
    for order in (kind, kind[np.argsort(perm)]):
        for tenth in np.array_split(order, 10):
            assert set(tenth.tolist()) == {0, 1, 2}
    by_slot = kind[np.argsort(perm)]
    assert by_slot[0] == 2 and by_slot[-1] == 2
    # a visited slot's neighbours are sentinels or the other component about as often as the parts' sizes say
    other = (by_slot[1:] != by_slot[:-1]) & (by_slot[:-1] != 2)
    assert other.sum() / (by_slot[:-1] != 2).sum() > 0.3


@pytest.mark.parametrize("form", list(FORMS_1D))
def test_oracle_1d_stays_inside_the_bound(form):
    before, after, updates = _oracle_1d_team() if form == "team" else _oracle_run(0, STREAMS, **FORMS_1D[form])
    rows = check(before, after, _graph()[0], 0, updates, case=f"oracle-1d-{form}")
    assert len(rows) == 2


@pytest.mark.parametrize("dims", list(FORMS_ND))
def test_oracle_layout_mirror_stays_inside_the_bound(dims):
    before, after, updates = _oracle_run(dims, STREAMS, **FORMS_ND[dims])
    rows = check(before, after, _graph()[0], dims, updates, case=f"oracle-D{dims}-team")
    assert len(rows) == 2 * dims


@pytest.mark.parametrize("switch,off", [("twin_trip", False), ("fused_trip", False), ("partners", 1)])
def test_special_trip_forms_are_reached_on_one_wave(switch, off):
    """One wave of the 1D mirror at the GPU cases' configuration: switching a trip form off changes the positions, so the form
    is taken on this graph (a form that is never taken leaves them bit-identical)."""
    _, on_x, _ = _oracle_run(0, 64, **TEAM_1D)
    _, off_x, _ = _oracle_run(0, 64, **dict(TEAM_1D, **{switch: off}))
    differ = int((on_x.view(np.uint64) != off_x.view(np.uint64)).sum())
    print(f"{switch}: {differ} of {on_x.shape[0]} words differ from the run with {switch}={off}")
    assert differ > 0


def test_two_partners_and_twin_trips_are_reached_in_the_layout_mirror(dims=2):
    form = FORMS_ND[dims]
    _, on_c, _ = _oracle_run(dims, 64, **form)
    for name, other in (("partners=1", dict(form, partners=1)), ("twin_trip=False", dict(form, twin_trip=False))):
        _, off_c, _ = _oracle_run(dims, 64, **other)
        differ = int((on_c.view(np.uint64) != off_c.view(np.uint64)).sum())
        print(f"D={dims} {name}: {differ} of {on_c.shape[0]} words differ")
        assert differ > 0


# ---- the checker fails on corrupted output ----------------------------------------------------------------------------------
def test_checker_catches_one_wrong_word():
    g, _ = _graph()
    before, after, updates = _oracle_1d_team()
    bad = after.copy()
    bad[g.components["A"][1234]] += 1e-3
    with pytest.raises(AssertionError, match="'A'"):
        check(before, bad, g, 0, updates, case="injected-1e-3")


def test_checker_catches_one_flipped_sentinel_bit():
    g, _ = _graph()
    before, after, updates = _oracle_1d_team()
    bad = after.copy()
    bad.view(np.uint64)[g.sentinels[77]] ^= np.uint64(1)
    with pytest.raises(AssertionError, match="sentinel"):
        check(before, bad, g, 0, updates, case="injected-sentinel-bit")


def test_checker_catches_an_add_moved_to_the_other_component():
    """The +r of one update lands on a node of B instead of its node of A: the sum over all nodes is kept (to rounding), the
    sums of A and of B are not."""
    g, _ = _graph()
    before, after, updates = _oracle_1d_team()
    r = 0.25
    bad = after.copy()
    bad[g.components["A"][10]] -= r
    bad[g.components["B"][10]] += r
    with pytest.raises(AssertionError, match="'A'"):
        check(before, bad, g, 0, updates, case="injected-misplaced-add")
    whole = type(g)(**{f: getattr(g, f) for f in g.__dataclass_fields__})      # the same graph as one component
    visited = np.concatenate([g.components["A"], g.components["B"]])
    whole.components, whole.sentinels = {"all": visited}, g.sentinels
    check(before, bad, whole, 0, updates, case="injected-misplaced-add-global-sum")


def test_checker_catches_a_layout_add_in_the_neighbouring_plane():
    g, _ = _graph()
    before, after, updates = _oracle_run(2, STREAMS, **FORMS_ND[2])
    bad = after.reshape(g.n_nodes, 2, 2).copy()
    node = g.components["B"][5]
    bad[node, 1, 0] -= 0.5                                                      # an add meant for dimension 0 ...
    bad[node, 1, 1] += 0.5                                                      # ... went to dimension 1 of the same end
    with pytest.raises(AssertionError, match="'B'"):
        check(before, bad.reshape(-1), g, 2, updates, case="injected-wrong-plane")
