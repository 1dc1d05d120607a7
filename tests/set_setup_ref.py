"""What the set-setup tests share (test_set_setup_host.py, test_gpu_set_setup.py): a numpy restatement of how a context's RNG
streams are seeded, and the sizes of the state arrays of a set-up context."""
import numpy as np

from gfasort_amd import hip

MASK = (1 << 64) - 1
COUNTER_BYTES = 1024 * 8 * 8                         # sgd_limits.h COUNTER_SLOTS lines of 8 u64
ITER_CONSTS_BYTES = 48


def seeded_words(seed, stream_base, n_streams):
    """The RNG words of a context set up with `seed` and `stream_base`, as they lie on the device: word k of stream t at
    [k * n_streams + t].  Stream t is Xoshiro256Plus::seed_from_u64(seed + stream_base + t) (sgd.rs:431-432), which is four
    successive SplitMix64 outputs; every sum and product wraps at 2^64 (numpy's uint64 arrays do)."""
    s = np.array([seed & MASK], dtype=np.uint64) + np.array([stream_base & MASK], dtype=np.uint64) + np.arange(n_streams, dtype=np.uint64)
    out = np.zeros((4, n_streams), dtype=np.uint64)
    for k in range(4):
        s = s + np.uint64(0x9E3779B97F4A7C15)
        z = (s ^ (s >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        out[k] = z ^ (z >> np.uint64(31))
    return out.reshape(-1)


def seeded_words_by_ints(seed, stream_base, n_streams):
    """The same rule in Python integers, masked by hand: one stream at a time, as capi.hip seed_streams walks them."""
    out = [0] * (4 * n_streams)
    for t in range(n_streams):
        s = (seed + stream_base + t) & MASK
        for k in range(4):
            s = (s + 0x9E3779B97F4A7C15) & MASK
            z = s
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
            out[k * n_streams + t] = z ^ (z >> 31)
    return np.array(out, dtype=np.uint64)


def all_states(ctx):
    """Every state array of a set-up context, as bytes, by kind."""
    return [ctx.debug_sgd_state(k).tobytes() for k in range(hip.STATE_KINDS)]
