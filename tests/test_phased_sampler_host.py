"""GFS_F_PHASED on the host (no GPU): the default window of gfs_phase_window, the ABI's constants and symbols, refusals that
need no device, and the CLI's `--phased-sampler`."""
import ctypes as C
import subprocess
import types

import pytest

from util import G, P, DATA
from gfasort_amd import build as B
from gfasort_amd import hip


def _params(iter_max, cooling_start):
    return types.SimpleNamespace(iter_max=iter_max, iter_with_max_learning_rate=0, min_term_updates=100, delta=0.0, eps=0.01,
                                 eta_max=100.0, theta=0.99, space=10, space_max=10, space_quantization_step=100,
                                 cooling_start=cooling_start, nthreads=1, seed=9399220, progress=False)


@pytest.mark.parametrize("iter_max", [0, 1, 2, 3, 100, 300, 10**6, 2**40, 2**64 - 1])
@pytest.mark.parametrize("cooling_start", [0.0, 0.25, 0.5, 0.9, 1.0, 2.0])
def test_default_window_lies_in_the_schedule(iter_max, cooling_start):
    b, e = hip.phase_window(_params(iter_max, cooling_start))
    assert 0 <= b <= e <= min(iter_max + 1, 2**64 - 1)
    assert (b, e) == hip.phase_window(_params(iter_max, cooling_start))           # a pure function


def test_default_window_follows_the_cooling_switch_and_scales_with_iter_max():
    f = lambda n, cs=0.5: int(n * cs)                                             # first_cooling = floor(cooling_start * iter_max)
    for n in (100, 300, 1000):
        b, e = hip.phase_window(_params(n, 0.5))
        assert b <= f(n) + 1 < e                                                  # the first cooling iteration is in the window
        b1, e1 = hip.phase_window(_params(n, 0.8))
        assert (b1, e1) != (b, e) and b1 <= f(n, 0.8) + 1 < e1
    (b1, e1), (b3, e3) = hip.phase_window(_params(100, 0.5)), hip.phase_window(_params(300, 0.5))
    assert abs((e3 - b3) - 3 * (e1 - b1)) <= 3                                    # a fraction of the schedule
    # the CLI's parameters on the reference's fixture
    g = G.load_gfa(f"{DATA}/DRB1-3123.gfa")
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    b, e = hip.phase_window(p)
    assert 0 < b <= int(p.cooling_start * p.iter_max) + 1 < e <= p.iter_max + 1


def test_constants_and_symbols():
    assert hip.F_PHASED == 0x40
    assert hip.F_PHASED & (hip.F_PLAIN_LOADS | hip.F_NO_LDS_TABLES | hip.F_NO_FUSE | hip.F_ONE_PARTNER | hip.F_DBG_FREE_RUNNING) == 0
    assert hip.F_PHASED & 0xFF00 == 0 and hip.F_PHASED & hip.F_BUNDLE(0xFF) == 0 and hip.F_PHASED & hip.F_CHAIN(0xFF) == 0
    L = hip.lib()
    for name in ("gfs_phase_window", "gfs_ctx_phase_window"):
        assert hasattr(L, name)
    with open(f"{B.CSRC}/../../include/gfasort_hip.h") as fh:
        h = fh.read()
    assert "#define GFS_F_PHASED        0x40u" in h and "int   gfs_phase_window(" in h and "int   gfs_ctx_phase_window(" in h


def test_calls_without_a_device_refuse_null_arguments():
    L = hip.lib()
    b, e = C.c_uint64(7), C.c_uint64(7)
    assert L.gfs_ctx_phase_window(None, -1, -1, C.byref(b), C.byref(e)) == hip.GfsError(-1, "").code == -1
    assert L.gfs_ctx_phase_window(None, 0, 1, None, None) == -1
    assert L.gfs_phase_window(None, C.byref(b), C.byref(e)) == -1
    sp = hip.make_sgd_params(_params(100, 0.5))
    assert L.gfs_phase_window(C.byref(sp), None, C.byref(e)) == -1
    assert (b.value, e.value) == (7, 7)


def test_rank_create_refuses_the_phased_sampler():
    g = G.synth_chain(2000, 1)
    p = P.YgsParams.from_graph(g, 0, 1).path_sgd
    with pytest.raises(hip.GfsError) as ei:
        hip.Rank(g, p, 0, 0, 1, launch=hip.make_config(flags=hip.F_PHASED))
    assert ei.value.code == -1 and "GFS_F_PHASED" in str(ei.value)


@pytest.fixture(scope="module")
def cli():
    B.build_host()
    return B.CLI


def test_cli_help_lists_the_flag(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--phased-sampler" in r.stderr and "cooling" in r.stderr


@pytest.mark.parametrize("extra", [["--reference-sampler"], ["--bundle", "1"], ["--bundle", "32"], ["--bundle", "16"]])
def test_cli_refuses_conflicting_samplers(cli, tmp_path, extra):
    o = str(tmp_path / "o.gfa")
    r = subprocess.run([cli, "-i", f"{DATA}/DRB1-3123.gfa", "-o", o, "-p", "Y", "--phased-sampler"] + extra,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--phased-sampler" in r.stderr
    for ok in (["--bundle", "auto"], ["--bundle", "64"]):                      # accepted by the parser (then: no device here)
        r = subprocess.run([cli, "-i", f"{DATA}/missing.gfa", "-o", o, "-p", "Y", "--phased-sampler"] + ok,
                           capture_output=True, text=True, timeout=60)
        assert "--phased-sampler" not in r.stderr
