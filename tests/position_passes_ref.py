"""The one-off position passes of a single context (csrc/index_kernels.hip) restated on the host, for
tests/test_gpu_position_passes.py: the ABI order <-> device order of positions and coordinates (reorder_positions_kernel), K4's
start positions as an integer prefix sum, K6's rank order as a lexsort — and the inputs that make a misplaced element name
itself.  Nothing here runs a kernel; tests/test_position_passes_host.py holds each restatement to a pure-Python loop."""
import numpy as np

from gfasort_amd import graph as G

EDGE_SIZES = (1, 2, 63, 64, 65, 257)
SEAM = 300_007            # past the 1024 x 256 = 262 144 threads of K4's and K6's own kernels; no multiple of 64
SEAM_1D_COPY = 600_011    # past the 2048 x 256 = 524 288 threads of reorder_positions_kernel at one element per node

# ---- doubles that say where they came from ---------------------------------------------------------------------------------
# a mark: sign 0, exponent 0x400 | tag (finite, normal), mantissa = index << 8 | end << 4 | dim.  No two marks of one vector are
# equal, and none equals a special below.
_SPECIALS = np.array([0x8000000000000000, 0x0000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
                      0x7FF8000000000000, 0xFFF8000000000123, 0x7FF0000000000001], dtype=np.uint64)   # -0, +0, +inf, -inf, 5e-324, NaNs


def marks(index, end, dim, tag):
    """The bit patterns (uint64) of the marks (index, end, dim) of pattern `tag` (1..255)."""
    assert 0 < tag < 256
    index, end, dim = (np.asarray(a, dtype=np.uint64) for a in (index, end, dim))
    return (np.uint64((0x400 | tag) << 52) | (index << np.uint64(8)) | (end << np.uint64(4)) | dim).astype(np.uint64)


def describe(word):
    """What the bits of one element say it was."""
    w = int(word)
    if (w >> 60) == 0x4 and ((w >> 52) & 0xFF):
        return "mark (index %d, end %d, dim %d) of pattern %d" % ((w >> 8) & ((1 << 44) - 1), (w >> 4) & 0xF, w & 0xF, (w >> 52) & 0xFF)
    return "no mark: " + plain(w)


def _with_specials(bits, seed):
    """Some elements replaced by both zeros, both infinities, a denormal and NaNs with payloads, where there is room."""
    if bits.shape[0] >= 2 * _SPECIALS.shape[0]:
        picks = np.random.default_rng(seed).permutation(bits.shape[0])[:_SPECIALS.shape[0]]
        bits[picks] = _SPECIALS
    return bits


def abi_pattern(n, dims, tag, seed=11):
    """A vector in the ABI's order, as float64: element (k*2 + end)*D + dim (1D: k) is the mark (k, end, dim)."""
    if dims == 0:
        bits = marks(np.arange(n), 0, 0, tag)
    else:
        k, end, dim = np.meshgrid(np.arange(n), np.arange(2), np.arange(dims), indexing="ij")
        bits = marks(k.reshape(-1), end.reshape(-1), dim.reshape(-1), tag)
    return _with_specials(bits, seed).view(np.float64)


def device_pattern(n, dims, tag, seed=12):
    """A vector in the device's order, as float64: element (end*D + dim)*N + slot (1D: slot) is the mark (slot, end, dim)."""
    if dims == 0:
        bits = marks(np.arange(n), 0, 0, tag)
    else:
        end, dim, slot = np.meshgrid(np.arange(2), np.arange(dims), np.arange(n), indexing="ij")
        bits = marks(slot.reshape(-1), end.reshape(-1), dim.reshape(-1), tag)
    return _with_specials(bits, seed).view(np.float64)


# ---- the order of positions on the device (sgd_device.h coord_ptr) --------------------------------------------------------
def to_device(v, perm, dims):
    """dev[(end*D + dim)*N + perm[k]] = v[(k*2 + end)*D + dim]; 1D (dims = 0): dev[perm[k]] = v[k].  Bits are kept."""
    perm = np.asarray(perm, dtype=np.int64)
    n, w = perm.shape[0], (2 * dims if dims else 1)
    src = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64).reshape(n, w)
    dev = np.empty((w, n), dtype=np.uint64)
    dev[:, perm] = src.T
    return dev.reshape(-1).view(np.float64)


def to_abi(dev, perm, dims):
    """The inverse: v[(k*2 + end)*D + dim] = dev[(end*D + dim)*N + perm[k]]; 1D: v[k] = dev[perm[k]]."""
    perm = np.asarray(perm, dtype=np.int64)
    n, w = perm.shape[0], (2 * dims if dims else 1)
    src = np.ascontiguousarray(dev, dtype=np.float64).view(np.uint64).reshape(w, n)
    return np.ascontiguousarray(src[:, perm].T).reshape(-1).view(np.float64)


def plain(word):
    w = int(word)
    return "0x%016x (%r)" % (w, np.array([w], dtype=np.uint64).view(np.float64)[0])


def first_difference(got, want, space, n, dims, marked=True):
    """None where got and want are bit-equal float64 vectors, else a text that names the first differing element, where it
    lies (`space`: "device" or "abi") and what the bits found there say they were (marked: the vectors hold marks)."""
    say = describe if marked else plain
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    gb, wb = got.view(np.uint64), want.view(np.uint64)
    bad = np.flatnonzero(gb != wb)
    if bad.size == 0:
        return None
    i = int(bad[0])
    if dims == 0:
        where = "%s element %d" % (space, i)
    elif space == "device":
        where = "device element %d = (end %d, dim %d, slot %d)" % (i, i // n // dims, i // n % dims, i % n)
    else:
        where = "abi element %d = (node %d, end %d, dim %d)" % (i, i // (2 * dims), i // dims % 2, i % dims)
    return "D = %d, N = %d: %d of %d elements differ, the first is %s: found %s, expected %s" % (
        dims, n, bad.size, gb.shape[0], where, say(gb[i]), say(wb[i]))


# ---- K4: the start positions ------------------------------------------------------------------------------------------------
def prefix_positions(node_len):
    """x[k] = sum of node_len[0..k) as an integer, then converted (sgd.rs:286-294 accumulates in usize and converts)."""
    return prefix_sums(node_len).astype(np.float64)                      # (uint64 -> f64 rounds to nearest, ties to even)


def prefix_sums(node_len):
    """The same sums as integers (uint64; never through a double: np.concatenate of an int list and a uint64 array would)."""
    node_len = np.asarray(node_len)
    sums = np.zeros(node_len.shape[0], dtype=np.uint64)
    sums[1:] = np.cumsum(node_len.astype(np.uint64))[:-1]
    return sums


# ---- K6: the rank order -----------------------------------------------------------------------------------------------------
def sort_reference(x):
    """order[r] = dense index of the node of rank r: ascending, -0.0 equal to +0.0, ties by dense index, every NaN last in
    dense order whatever its sign or payload (sgd.rs:665-671 with the NaN rule of gfs_sort_order)."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):                                  # (a signalling NaN + 0.0)
        keys = np.where(nan, np.inf, x + 0.0)
    return np.lexsort((np.arange(x.shape[0]), nan, keys)).astype(np.uint64)


_NANS = np.array([0x7FF8000000000000, 0xFFF8000000000123, 0x7FF0000000000001, 0xFFF0000000000001, 0xFFFFFFFFFFFFFFFF],
                 dtype=np.uint64).view(np.float64)
_ODD_VALUES = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.0 ** -1060, -1.0, -3.5, 7.25], dtype=np.float64)


def hostile_positions(n, seed):
    """Multiples of 8 of both signs, about 16 nodes to a value, and sprinkled among them NaNs of both signs and with payloads,
    both zeros (also a run of them interleaved in dense order), both infinities, denormals of both signs and negatives."""
    assert n >= 64
    rng = np.random.default_rng(seed)
    half = max(n // 32, 2)
    x = 8.0 * rng.integers(-half, half, n).astype(np.float64)
    reps = max(1, min(40, n // 64))
    odd = np.concatenate([_NANS, _ODD_VALUES])
    picks = rng.permutation(n)[:odd.shape[0] * reps]
    xb, ob = x.view(np.uint64), np.tile(odd, reps).view(np.uint64)
    xb[picks] = ob                                                     # (as bits: a NaN keeps its sign and payload)
    a = int(rng.integers(0, n - 16))
    x[a:a + 16:2], x[a + 1:a + 16:2] = 0.0, -0.0
    return x


# ---- graphs and layouts -----------------------------------------------------------------------------------------------------
def chain_under_two_paths(n, node_len, seed=3, steps_per_path=None):
    """graph.py's window graph with two paths over a chain of n nodes (both over the whole chain, or of `steps_per_path` steps at
    its two ends), S lines block-shuffled so that path order is not the dense order, and node_len overwritten."""
    g = G.synth_windows(n, 2, min(n, steps_per_path or n), seed)
    node_len = np.ascontiguousarray(node_len, dtype=np.uint32)
    assert node_len.shape == (n,)
    g.node_len = node_len
    return g


def random_layout(n, seed, avoid=()):
    """A seeded random permutation that is neither the identity nor any of `avoid` (where n leaves a third choice; at n = 2
    only the identity is avoided, at n = 1 there is one layout)."""
    rng = np.random.default_rng(seed)
    ident = np.arange(n, dtype=np.uint32)
    perm = ident
    for _ in range(64):
        perm = rng.permutation(n).astype(np.uint32)
        if n < 2 or (not np.array_equal(perm, ident) and (n == 2 or not any(np.array_equal(perm, a) for a in avoid))):
            break
    return perm


def mixed_lengths(n, seed):
    """Lengths 1..16 with one node in seven of length 0 (so runs of them occur), zero-length nodes in the first and last place."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 17, n).astype(np.uint32)
    lens[rng.random(n) < 1.0 / 7.0] = 0
    lens[0] = lens[-1] = 0
    return lens


def huge_lengths(n, seed):
    """Lengths up to 2^32 - 1, that value among the first: the partial sums cross 2^32 within the first few nodes."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    lens[:min(n, 3)] = 0xFFFFFFFF
    if n > 8:
        lens[n // 2] = 0xFFFFFFFF
    return lens
