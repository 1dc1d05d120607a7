"""What gfs_ctx_setup_1d / _nd, gfs_ctx_reset_streams and gfs_ctx_phase_window leave on the device, as digests: for a fixed list of
cases the return code, the facts the ABI shows of the setup (tests/test_gpu_set_setup.py _facts) and the SHA-256 of each of the
eight state arrays (Context.debug_sgd_state).  Every case fixes n_streams in its launch config, so no digest depends on the
residency query; integer arithmetic and host tables only, so the digests are the same on every run.

    python scripts/setup_state_digest.py > tests/golden/setup_state_digests.json

tests/golden/setup_state_digests.json was produced by this script at commit fe1c79e ("Team sort trips at B = 64 read 8-byte trip
records"), the last one whose single setup had a device-side text of its own (capi.hip setup_common: a host loop over the streams,
a blocking copy per table, an allocation per array); tests/test_gpu_setup_digests.py recomputes the digests and compares them, so
the single setup that is a set setup of one item is held to the bits of the text it replaced, not to itself.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

from gfasort_amd import hip  # noqa: E402
from util import load  # noqa: E402
from test_gpu_set_setup import _mix, _base_1d, _base_nd, _with, _facts  # noqa: E402
from test_gpu_trip_records import mixed_graph, _ygs  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def snapshot(ctx, rc, kinds=range(hip.STATE_KINDS)):
    """One record: the return code, the facts, and per state array its digest and its bytes (None for a kind left out)."""
    arrays = [ctx.debug_sgd_state(k) if k in kinds else None for k in range(hip.STATE_KINDS)]
    return {"rc": int(rc), "facts": list(_facts(ctx, rc)),
            "bytes": [None if a is None else int(a.nbytes) for a in arrays],
            "sha256": [None if a is None else sha(a) for a in arrays]}


def _setup(ctx, p, cfg, dims, **tables):
    return ctx.setup_1d(p, cfg, **tables) if dims == 0 else ctx.setup_nd(p, cfg, **tables)


def case_mix(dims):
    """Every item of the set tests' mix, set up alone: the fixtures, 0 nodes, one-step paths, 255 / 256 / 257 streams, one stream,
    the seed 2^64 - 2, the stream base 2^64 - 100."""
    base = _base_1d() if dims == 0 else _base_nd(dims)
    out = []
    for g, seed, cfg in _mix():
        if cfg is None:
            cfg = hip.make_config(n_streams=70)                         # (the mix leaves some to the policy: fixed here)
        ctx = hip.Context(g)
        try:
            out.append(snapshot(ctx, _setup(ctx, _with(base, seed=seed), cfg, dims)))
        finally:
            ctx.close()
    return out


def _team_params(g):
    return _ygs(g, 20, 20_000)


def case_team(trace_per_stream):
    """Bundles of 64 on one wave: team state, and with tracing the trace buffers and their counts."""
    g = mixed_graph()
    ctx = hip.Context(g)
    try:
        cfg = hip.make_config(n_streams=64, flags=hip.F_BUNDLE(64), trace_per_stream=trace_per_stream)
        return [snapshot(ctx, ctx.setup_1d(_team_params(g), cfg))]
    finally:
        ctx.close()


def case_phased():
    """GFS_F_PHASED, then the window moved: the resident schedule table carries the window's marks and goes up again."""
    g = mixed_graph()
    ctx = hip.Context(g)
    try:
        rc = ctx.setup_1d(_team_params(g), hip.make_config(n_streams=64, flags=hip.F_PHASED | hip.F_BUNDLE(64)))
        out = [snapshot(ctx, rc)]
        before = ctx.phase_window()
        assert ctx.phase_window(2, 5) == (2, 5) != before
        out.append(snapshot(ctx, rc))
        assert out[0]["sha256"][hip.STATE_SCHEDULE] != out[1]["sha256"][hip.STATE_SCHEDULE]
        return out
    finally:
        ctx.close()


def caller_tables():
    """(params, launch config, [(etas, zetas)] of the three setups with caller-supplied tables) on DRB1-3123."""
    p = _with(_base_1d(iter_max=9), seed=77)
    etas, zetas = hip.sgd_schedule(p), hip.zeta_table(p)
    return p, hip.make_config(n_streams=70), [(etas, zetas), (etas * 0.5, zetas), (etas, np.ones_like(zetas))]


def case_caller_tables():
    p, cfg, tables = caller_tables()
    ctx = hip.Context(load("DRB1-3123.gfa"))
    try:
        return [snapshot(ctx, ctx.setup_1d(p, cfg, etas=etas, zetas=zetas)) for etas, zetas in tables]
    finally:
        ctx.close()


def case_refused():
    """A launch shape the policy refuses (tests/test_gpu_set_setup.py): the error, and what is left — the zeroed replica alone."""
    g = load("lil.gfa")
    ctx = hip.Context(g)
    try:
        out = {}
        try:
            ctx.setup_1d(_base_1d(), hip.make_config(n_streams=1, block_size=100))
            out["rc"] = 0
        except hip.GfsError as e:
            out["rc"], out["error"] = int(e.code), str(e)
        out["positions_len"] = ctx.positions_len()
        out["has_positions"] = bool(ctx.positions_device())
        x = ctx.download()
        out["positions_zero"] = not x.any()
        out["positions_sha256"] = sha(x)
        out["n_streams"] = int(ctx.stats().n_streams)
        for name, call in (("state", lambda: ctx.debug_sgd_state(hip.STATE_RNG)), ("reset", ctx.reset_streams), ("run", ctx.run)):
            try:
                call()
                out[name] = None
            except hip.GfsError as e:
                out[name] = [int(e.code), str(e)]
        return [out]
    finally:
        ctx.close()


def case_reset_one_stream():
    """One stream with a trace: setup, two iterations, reset_streams.  RNG words, counters and trace counts are a fresh setup's;
    the positions and the traces are those of the run."""
    g = load("DRB1-3123.gfa")
    p = _with(_base_1d(iter_max=4, updates=1500), seed=55)
    ctx = hip.Context(g)
    try:
        rc = ctx.setup_1d(p, hip.make_config(n_streams=1, trace_per_stream=3))
        out = [snapshot(ctx, rc)]
        ctx.init_positions()
        ctx.run_range([0, 1])
        ctx.synchronize()
        out.append(snapshot(ctx, rc))
        ctx.reset_streams()
        out.append(snapshot(ctx, rc))
        assert out[1]["sha256"][hip.STATE_POSITIONS] == out[2]["sha256"][hip.STATE_POSITIONS] != out[0]["sha256"][hip.STATE_POSITIONS]
        assert out[1]["sha256"][hip.STATE_RNG] != out[0]["sha256"][hip.STATE_RNG]
        return out
    finally:
        ctx.close()


def case_reset_team():
    """A wave of bundles of 64: setup, two iterations, reset_streams; everything but the positions."""
    g = mixed_graph()
    kinds = range(1, hip.STATE_KINDS)
    ctx = hip.Context(g)
    try:
        rc = ctx.setup_1d(_team_params(g), hip.make_config(n_streams=64, flags=hip.F_BUNDLE(64)))
        out = [snapshot(ctx, rc, kinds)]
        ctx.init_positions()
        ctx.run_range([0, 1])
        ctx.synchronize()
        ran = snapshot(ctx, rc, kinds)                                  # (not recorded: only that the run left something to reset)
        for kind in (hip.STATE_LEAD, hip.STATE_COUNTERS, hip.STATE_RNG):
            assert ran["sha256"][kind] != out[0]["sha256"][kind], kind
        ctx.reset_streams()
        out.append(snapshot(ctx, rc, kinds))
        return out
    finally:
        ctx.close()


def case_again():
    """1D, then 2-D, then 1D on one context."""
    g = load("DRB1-3123.gfa")
    cfg = hip.make_config(n_streams=257)
    ctx = hip.Context(g)
    try:
        return [snapshot(ctx, _setup(ctx, _with(_base_1d() if dims == 0 else _base_nd(dims), seed=600 + dims), cfg, dims)) for dims in (0, 2, 0)]
    finally:
        ctx.close()


CASES = {
    "mix D=0": lambda: case_mix(0), "mix D=2": lambda: case_mix(2), "mix D=3": lambda: case_mix(3), "mix D=8": lambda: case_mix(8),
    "team": lambda: case_team(0), "team traced": lambda: case_team(2), "phased, window moved": case_phased,
    "caller's etas and zetas": case_caller_tables, "refused by the launch policy": case_refused,
    "reset, one stream": case_reset_one_stream, "reset, team": case_reset_team, "1D, 2-D, 1D": case_again,
}


def main():
    json.dump({name: case() for name, case in CASES.items()}, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
