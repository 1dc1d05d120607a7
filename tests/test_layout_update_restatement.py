"""The arithmetic of one layout update, restated independently of the oracle.

The oracle's nD update (oracle/gfs_oracle.c term_nd_ck) is project code and the golden file is generated from it; the sampler
pieces have Python restatements in test_oracle_kat.py, the update had none.  util.replay_layout_trace is one: sgd.rs:1085-1149
as read from the reference, in plain Python floats.  Here the oracle's single-stream run is traced in full and the replay of
that trace must give the oracle's final coordinates bit for bit, at every D = 1..8.  The all-zero start drives the
mag_sq == 0 branch (sgd.rs:1116-1119) on the first touch of every pair, the self-loop path the i == j store order
(sgd.rs:1143-1149).

The replay has no crowding term (the reference has none; it is the product's).  Single-stream runs hand the kernels
kshift = floor(log2(n_steps / 2)) + 2, above every exponent of these fixtures; asserted, not assumed.

Mutations tried on a scratch copy of the replay (each must turn at least one case red):
  i == j store order swapped       -> the 3 self-loop cases fail; the 16 DRB1 cases pass (DRB1 has no i == j term)
  mag_sq == 0 substitution dropped -> the 8 all-zero DRB1 cases and the 3 self-loop cases fail (r = 0 / 0; an i == j term has
                                      mag_sq == 0 too); the 8 Gaussian DRB1 cases pass
  mag_sq summed right to left      -> the Gaussian DRB1 cases fail at D = 3..8 and the self-loop cases at D = 5, 8; D = 1, 2 pass
                                      (a sum of two terms has one order), and so does every all-zero start (there the
                                      dimensions k >= 1 stay zero for good, so the sum has one non-zero term)
"""
import numpy as np
import pytest

from util import (O, P, load, oracle_graph, oracle_params, gaussian_init, replay_layout_trace, np_crowding, self_loop_graph,
                  single_stream_kshift)


def _traced_oracle_run(g, dims, iter_max, min_term_updates, c0):
    p = P.LayoutSGDParams.from_graph(g, dims, 1)
    p.iter_max = iter_max
    if min_term_updates:
        p.min_term_updates = min_term_updates
    og, op = oracle_graph(g), oracle_params(p)
    total = (p.iter_max + 1) * p.min_term_updates
    c_ref = c0.copy()
    rc, st, tr = O.sgd_nd(og, op, c_ref, n_streams=1, trace_per_stream=total)
    assert rc == 0
    # what makes the replay legitimate: every iteration does exactly min_term_updates updates and all of them are traced,
    # so the n-th traced term ran in iteration n // min_term_updates
    assert st.term_updates == total and st.attempts >= total
    assert tr.shape[0] == total and (tr["d_ij"] > 0.0).all()
    # ... and no crowding: every exponent is below the onset of a one-stream run
    _, _, a, _ = np_crowding(g)
    assert a.max() < single_stream_kshift(g)
    return p, O.schedule(op), tr, c_ref, st


@pytest.mark.parametrize("start", ["gaussian", "zeros"])
@pytest.mark.parametrize("dims", [1, 2, 3, 4, 5, 6, 7, 8])
def test_replay_of_the_oracle_trace_equals_the_oracle_on_drb1(dims, start):
    g = load("DRB1-3123.gfa")
    c0 = gaussian_init(g, dims, 7) if start == "gaussian" else np.zeros(g.n_nodes * 2 * dims, dtype=np.float64)
    p, etas, tr, c_ref, st = _traced_oracle_run(g, dims, 3, 20000, c0)
    assert (st.term_updates, st.attempts) == (80000, 82495)          # the sampler does not read coordinates
    if start == "zeros":
        # the first touch of a pair of untouched ends has mag_sq == 0; the run's first term is such a pair at any D
        assert not c0.any()
    c = replay_layout_trace(c0, dims, tr, etas, p.min_term_updates)
    assert np.isfinite(c_ref).all()
    assert np.array_equal(c.view(np.uint64), c_ref.view(np.uint64))


@pytest.mark.parametrize("dims", [1, 5, 8])
def test_replay_of_the_oracle_trace_equals_the_oracle_on_a_self_loop_path(dims):
    g = self_loop_graph()
    c0 = gaussian_init(g, dims, 3)
    p, etas, tr, c_ref, st = _traced_oracle_run(g, dims, 20, 0, c0)
    assert int((tr["i"] == tr["j"]).sum()) >= 1                      # the 'second store wins' case occurs
    c = replay_layout_trace(c0, dims, tr, etas, p.min_term_updates)
    assert np.isfinite(c_ref).all()
    assert np.array_equal(c.view(np.uint64), c_ref.view(np.uint64))
