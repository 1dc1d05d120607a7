"""The multi-rank run restated in numpy: W ranks run one after another in one process, no GPU and no torch.

What is restated is the merge of include/gfasort_hip.h ("multi-device runs") and DESIGN.md §6: the windows, the element
order of the exchange buffer, [delta | touched], the four divisor rules, `cscale`, the owned intervals and the re-snapshot
at the end.  What is NOT restated is taken from pieces other tests already pin: the plan from hip.ShardPlan (host only,
tests/test_host_logic.py), the learning rates from hip.sgd_schedule, and a rank's own term updates from the oracle's
resumable state at ONE reference stream (a rank's context at n_streams = 1 equals it bit for bit, tests/test_gpu_parity.py).

The element order is the wire format a host all-reduces, so it is written out here and not asked of the product:
  planes outermost, segments ascending, slots ascending; planes = 1 (1D) or 2 * D (nD), plane r = end * D + dim;
  element (plane r, slot s) is ABI index k (1D) or (k * 2 + end) * D + dim (nD) of the dense node k with perm[k] = s;
  the buffer is [delta(total) | touched(total)] in the payload type.

`eta_sum` = max(1, mean node length), the mean formed as the product forms it: a long-double sum divided by a long-double
count, rounded to double once.  A plain float64 division rounds the same quotient from its float64 operands, which can
differ in the last bit.  `mean_node_length` returns both; on none of the graphs of tests/multi_cases.py do they differ
(tests/test_multi_restatement_host.py asserts that, so a new graph where they do is noticed, not papered over)."""
import numpy as np

from util import O, oracle_graph, oracle_params
from gfasort_amd import hip
from gfasort_amd.distributed import SHARDING, subgraph

RULES = ("anneal", "sum", "mean", "touch")


def mean_node_length(g):
    """(as the product forms it, by a plain float64 division)."""
    n = g.n_nodes
    if n == 0:
        return 1.0, 1.0
    bp = g.node_len.astype(np.longdouble).sum()                     # integers below 2^64: exact in long double
    return float(bp / np.longdouble(n)), float(np.float64(int(g.node_len.astype(np.uint64).sum())) / np.float64(n))


def windows_of(ks, merge_every, iter_max):
    """Iterations ks cut into merge windows: one closes after every `merge_every` iterations counted from 0 and after
    iteration iter_max."""
    every, out, seg = max(1, int(merge_every)), [], []
    for k in ks:
        seg.append(int(k))
        if (int(k) + 1) % every == 0 or int(k) == int(iter_max):
            out.append(seg)
            seg = []
    assert not seg, "the iterations must end on a window's end"
    return out


def bits(a):
    """The bit patterns of a float32 / float64 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def hexval(v):
    return "0x%0*x" % (2 * v.dtype.itemsize, int(bits(np.array([v]))[0]))


class Cluster:
    """W ranks of one run.  After window() / finish() the lists `windows` and `finishes` hold what a test compares:
    windows[i]  = dict(ks, moves[rank] (float64, before the cast), bufs[rank] (before the sum), sum, cscale,
                       x[rank] (positions after the apply, ABI order))
    finishes[i] = dict(masked[rank] (ABI order), x (the final positions))"""

    def __init__(self, g, p, world, dims=0, merge="anneal", payload_f64=False, sharding="auto", whole_vector=False):
        assert world >= 2 and merge in RULES
        self.g, self.p, self.world, self.dims, self.merge = g, p, int(world), int(dims), merge
        self.T = np.float64 if payload_f64 else np.float32
        self.plan = plan = hip.ShardPlan(g, int(p.min_term_updates), world, SHARDING[sharding], whole_vector)
        self.quotas = [int(q) for q in plan.quotas]
        n, D = g.n_nodes, self.dims
        self.width = 2 * D if D else 1
        self.planes = self.width
        perm = plan.perm.astype(np.int64)
        self.node_of_slot = np.empty(n, dtype=np.int64)
        self.node_of_slot[perm] = np.arange(n)
        self.segments = [(int(lo), int(hi)) for lo, hi in plan.shared]
        # the exchange's element space
        self.elem_plane, self.elem_slot = self._elements(self.segments)
        self.elem_node = self.node_of_slot[self.elem_slot]
        self.idx = self._abi(self.elem_plane, self.elem_node)
        self.total = int(self.idx.shape[0])
        # the device's element space (every plane, every slot): what finish_begin fills
        dev_plane, dev_slot = self._elements([(0, n)] if n else [])
        self.abi_of_device = self._abi(dev_plane, self.node_of_slot[dev_slot])
        owner_of_slot = np.full(n, -1, dtype=np.int64)
        for lo, hi, r in plan.owned:
            owner_of_slot[lo:hi] = r
        assert (owner_of_slot >= 0).all(), "the owned intervals must tile the slots"
        self.owner_of_slot = owner_of_slot
        self.owner = np.repeat(owner_of_slot[perm], self.width)        # ABI order: a node's owner holds all its elements
        # the ranks
        first = g.path_first_step.astype(np.int64)
        self.etas = hip.sgd_schedule(p)
        self.eta_sum = max(1.0, mean_node_length(g)[0])
        self.states, self.idle, self._keep = [], [], []
        op = oracle_params(p)
        for r in range(self.world):
            paths = plan.paths_of(r)
            idle = self.quotas[r] == 0 or not any(first[q + 1] - first[q] > 1 for q in paths)
            self.idle.append(idle)
            if idle:
                self.states.append(None)
                continue
            og = oracle_graph(subgraph(g, paths))
            self._keep.append(og)
            self.states.append(O.State(og, op, dims=D, n_streams=1, stream_base=r, quota_total=self.quotas[r]))
        self.x = self.x_prev = None
        self.windows, self.finishes = [], []

    def _elements(self, segments):
        plane, slot = [], []
        for r in range(self.planes):
            for lo, hi in segments:
                plane.append(np.full(hi - lo, r, dtype=np.int64))
                slot.append(np.arange(lo, hi, dtype=np.int64))
        if not plane:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        return np.concatenate(plane), np.concatenate(slot)

    def _abi(self, plane, node):
        D = self.dims
        if D == 0:
            return node.copy()
        end, dim = plane // D, plane % D
        return (node * 2 + end) * D + dim

    def set_positions(self, x=None):
        """x: ABI order; None: the reference's start (1D)."""
        if x is None:
            assert self.dims == 0
            x = O.init_positions(oracle_graph(self.g))
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape[0] == self.g.n_nodes * self.width
        self.x = [x.copy() for _ in range(self.world)]
        self.x_prev = [v[self.idx].copy() for v in self.x]

    def window(self, ks):
        ks = [int(k) for k in ks]
        for r, st in enumerate(self.states):
            if not self.idle[r]:
                for k in ks:
                    st.run_iteration(k, self.x[r])
        T, total = self.T, self.total
        bufs, moves = [], []
        for r in range(self.world):
            d = self.x[r][self.idx] - self.x_prev[r]
            moves.append(d)
            with np.errstate(over="ignore"):
                bufs.append(np.concatenate([d.astype(T), (d != 0.0).astype(T)]))
        s = bufs[0].copy()
        for r in range(1, self.world):
            s = s + bufs[r]
        assert s.dtype == T
        c = s[total:].astype(np.float64)
        cscale = 1.0
        if self.merge == "anneal":
            cscale = min(1.0, float(len(ks)) * float(self.etas[ks[-1]]) / self.eta_sum)
            cc = c * cscale
            div = np.where(cc > 1.0, cc, 1.0)
        elif self.merge == "touch":
            div = np.where(c > 1.0, c, 1.0)
        else:
            div = np.full(total, 1.0 if self.merge == "sum" else float(self.world))
        step = s[:total].astype(np.float64) / div
        for r in range(self.world):
            self.x_prev[r] = self.x_prev[r] + step
            self.x[r][self.idx] = self.x_prev[r]
        rec = dict(ks=ks, moves=moves, bufs=bufs, sum=s, cscale=cscale, x=[v.copy() for v in self.x])
        self.windows.append(rec)
        return rec

    def finish(self):
        masked = [np.where(self.owner == r, self.x[r], 0.0) for r in range(self.world)]
        full = masked[0].copy()
        for r in range(1, self.world):
            full = full + masked[r]
        self.x = [full.copy() for _ in range(self.world)]
        self.x_prev = [v[self.idx].copy() for v in self.x]
        rec = dict(masked=masked, x=full.copy())
        self.finishes.append(rec)
        return rec

    def describe(self, e):
        """Exchange element e as (plane, slot, dense node)."""
        return int(self.elem_plane[e]), int(self.elem_slot[e]), int(self.elem_node[e])

    def describe_abi(self, i):
        """ABI index i as (plane, slot, dense node)."""
        D = self.dims
        node = i // self.width
        plane = 0 if D == 0 else ((i // D) % 2) * D + i % D
        return int(plane), int(self.plan.perm[node]), int(node)

    def close(self):
        for st in self.states:
            if st is not None:
                st.close()
