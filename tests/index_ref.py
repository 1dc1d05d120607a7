"""The index of a context restated on the host, for the tests that hold the device build to it (test_gpu_step_records.py,
test_gpu_ctx_set.py): the 16-byte step records (K3, format sgd_device.h) in numpy, and the node layout as the host's
gfs_shared_node_layout gives it (multi.hip, which tests/test_host_logic.py pins to a plain-loop restatement).  Neither runs a
kernel.  And the free device memory, for the tests that hold a failed create to leaving none behind."""
import ctypes as C
import gc

import numpy as np

from util import np_crowding, NO_NODE
from gfasort_amd import hip
from gfasort_amd.distributed import path_order_layout

POS_HI = 0x7FFFFF
FIELDS = ("node slot", "path | rev", "pos lo", "pos hi | a | b")


def np_records(g, perm, crowd=None):
    """K3 restated: rec[s] = {perm[n] | NO_NODE, path | rev << 31, pos lo, pos hi (23 bits) | a << 23 | b << 29}, padding zero."""
    S = g.n_steps
    sn = g.step_node.astype(np.int64)
    present = sn != NO_NODE
    pos, _ = g.step_positions()
    pos = pos.astype(np.uint64)
    _, _, a, b = crowd if crowd is not None else np_crowding(g)
    perm = np.asarray(perm, dtype=np.int64)
    if g.n_nodes == 0:                                                  # (nothing is present: the look-ups below select nothing)
        perm, a, b = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
    first = g.path_first_step.astype(np.int64)
    path = np.repeat(np.arange(g.n_paths, dtype=np.int64), np.diff(first))
    rec = np.zeros((S + 1, 4), dtype=np.uint32)
    safe = np.where(present, sn, 0)
    rec[:S, 0] = np.where(present, perm[safe], NO_NODE)
    rec[:S, 1] = (path | (g.step_is_rev.astype(np.int64) << 31)).astype(np.uint32)
    rec[:S, 2] = (pos & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    crowd_w = np.where(present, (a[safe] << 23) | (b[safe] << 29), 0)
    rec[:S, 3] = (((pos >> np.uint64(32)).astype(np.int64) & POS_HI) | crowd_w).astype(np.uint32)
    return rec


def same_records(rec, want, where=""):
    """Field by field, so that a failure names the field and the first steps; the padding record zero."""
    assert rec.shape == want.shape, where
    assert not rec[-1].any(), f"{where}: padding record not zero"
    for f, name in enumerate(FIELDS):
        bad = np.nonzero(rec[:, f] != want[:, f])[0]
        assert bad.size == 0, f"{where}: {name}: {bad.size} records differ, first at step {bad[:5]}: {rec[bad[:5], f]} != {want[bad[:5], f]}"


class HostIndex:
    """What a context of g must hold, computed once: the layout by the host's rule and the records with its slots."""

    def __init__(self, g):
        self.g = g
        self.crowd = np_crowding(g)
        self.layout = path_order_layout(g)
        self.records = np_records(g, self.layout, self.crowd)

    def check(self, ctx, where=""):
        assert np.array_equal(ctx.node_layout(), self.layout), f"{where}: node layout"
        same_records(ctx.step_records(), self.records, where)


def free_device_bytes():
    """Free device memory as hipMemGetInfo of the library's own runtime reports it (a symbol lookup on the library's handle
    searches its dependencies), with the device idle.  The figure is the whole device's, so whatever else this process still
    holds must not change between two samples: garbage of earlier tests (contexts in reference cycles free their device memory
    when the collector gets to them) is collected first."""
    gc.collect()
    L = hip.lib()
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.hipDeviceSynchronize.argtypes = []
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert L.hipDeviceSynchronize() == 0
    assert L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)
