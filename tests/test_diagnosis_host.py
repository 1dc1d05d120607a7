"""The localising read-outs' ABI (K7d, K7e, K7f) on a machine WITHOUT a GPU: the symbols are declared, exported and listed, the
argument errors that need no device are reported as such, the one-shot entry fails loudly, and the CLI documents its flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from util import ROOT, load
from gfasort_amd import build as B
from gfasort_amd import hip

NEW = ["gfs_ctx_path_errors", "gfs_ctx_stretched_pairs", "gfs_ctx_node_errors", "gfs_diagnose"]


def test_new_symbols_are_declared_exported_and_listed():
    with open(os.path.join(ROOT, "include", "gfasort_hip.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    L = hip.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in hip.EXPORTS, name
    for struct, dtype, words in (("gfs_path_error", hip.PATH_ERROR_DTYPE, 8), ("gfs_stretched_pair", hip.STRETCHED_PAIR_DTYPE, 5),
                                 ("gfs_node_error", hip.NODE_ERROR_DTYPE, 3)):
        m = re.search(r"typedef struct %s\s*\{(.*?)\}" % struct, hdr, flags=re.S)
        assert m, struct
        fields = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert fields == list(dtype.names) and dtype.itemsize == 8 * words, struct


def test_argument_errors_come_before_any_device_call():
    L, p = hip.lib(), hip._ptr
    g = load("simple.gfa")
    v, keep = hip.make_view(g)
    x = hip.init_positions(g)
    paths = np.zeros(g.n_paths, dtype=hip.PATH_ERROR_DTYPE)
    pairs = np.zeros(4, dtype=hip.STRETCHED_PAIR_DTYPE)
    t = C.c_uint64(5)
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 0, 10.0, p(paths), p(pairs), 4, C.byref(t)) == -1 and b"step distance of 0" in L.gfs_last_error()
    assert t.value == 0
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 1, float("nan"), p(paths), p(pairs), 4, C.byref(t)) == -1 and b"ratio" in L.gfs_last_error()
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 1, -0.5, p(paths), p(pairs), 4, C.byref(t)) == -1
    assert L.gfs_diagnose(None, 0, p(x), 1, 10.0, p(paths), p(pairs), 4, C.byref(t)) == -1
    assert L.gfs_diagnose(C.byref(v), 0, None, 1, 10.0, p(paths), p(pairs), 4, C.byref(t)) == -1
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 1, 10.0, None, p(pairs), 4, C.byref(t)) == -1
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 1, 10.0, p(paths), None, 4, C.byref(t)) == -1
    assert L.gfs_diagnose(C.byref(v), 0, p(x), 1, 10.0, p(paths), p(pairs), 4, None) == -1
    assert L.gfs_diagnose(C.byref(v), 9, p(x), 1, 10.0, p(paths), p(pairs), 4, C.byref(t)) == -1
    assert not pairs.view(np.uint64).any()
    # the context entries: a null context is an argument error
    assert L.gfs_ctx_path_errors(None, 1, 10.0, p(paths), g.n_paths, None) == -1
    assert L.gfs_ctx_stretched_pairs(None, 1, 10.0, p(pairs), 4, C.byref(t), None) == -1
    assert L.gfs_ctx_node_errors(None, 1, 10.0, p(pairs), g.n_nodes, None) == -1


@pytest.mark.skipif(hip.lib().gfs_device_count() > 0, reason="a GPU is present")
def test_one_shot_fails_loudly_without_gpu():
    g = load("simple.gfa")
    with pytest.raises(hip.GfsError) as ei:
        hip.diagnose(g, hip.init_positions(g))
    assert ei.value.code == -2 and "no CPU fallback" in str(ei.value)
    with pytest.raises(hip.GfsError) as ei:
        hip.diagnose(g, hip.init_layout(g, 2, 7), cap=0, dims=2)
    assert ei.value.code == -2


def test_usage_mentions_the_flags():
    B.build_host()
    r = subprocess.run([B.CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--diagnose" in r.stderr and "--diagnose-ratio R" in r.stderr
