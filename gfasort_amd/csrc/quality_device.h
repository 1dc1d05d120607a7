// quality_device.h — the device functions K7 (quality_kernels.hip) and its batch forms K7g (batch_quality_kernels.hip),
// K7h-j (batch_diagnosis_kernels.hip) and K7k (batch_sort_quality_kernels.hip) share: the one per-pair function, the fixed-tree
// reduction of a workgroup's five fields and the sum of an item's partials, K7c's pass over adjacent steps, and what a wave does
// with one tile, one path or one pair in K7d-f.  One text for all units, so that a batch's figures are
// the per-item call's bit for bit.
#pragma once
#include "batch_readout_plan.h"                           // Q_BLOCK, Q_PAIRS_PER_THREAD, Q_MAX_BLOCKS, Q_TILE, Q_TILE_ROUNDS
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gfs {

static constexpr uint32_t Q_NO_NODE = 0xFFFFFFFFu;

// ---- the one per-pair function (sgd.rs:1252-1275) ---------------------------------------------------------------------
// step record: { slot | NO_NODE, path | rev << 31, pos lo, pos hi (23 bits) | crowding exponents } (index_set_kernels.hip)
__device__ __forceinline__ uint64_t rec_pos(const uint4 r) { return (uint64_t)r.z | ((uint64_t)(r.w & 0x7FFFFFu) << 32); }
__device__ __forceinline__ uint32_t rec_path(const uint4 r) { return r.y & 0x7FFFFFFFu; }

// x: the context's position buffer in its own order — 1D x[slot] (dims = 0), nD the planes [end][dim][slot], of which the
// '+' end (end 0) is planes 0..dims-1.  False: the pair is skipped (another path, d_path == 0, an absent node).
__device__ __forceinline__ bool pair_error(const uint4 ra, const uint4 rb, const double *x, const uint64_t n_nodes, const uint32_t dims,
                                           double &err, double &rel_sq) {
    if (rec_path(ra) != rec_path(rb)) return false;
    const double d_path = fabs((double)rec_pos(ra) - (double)rec_pos(rb));   // :1252-1254
    if (d_path == 0.0) return false;                                         // :1256
    if (ra.x == Q_NO_NODE || rb.x == Q_NO_NODE) return false;                // :1260-1267
    double sum_sq = 0.0;                                                     // layout.rs:126-133
    const uint32_t terms = dims ? dims : 1u;
    for (uint32_t d = 0; d < terms; ++d) {
        const double delta = x[(uint64_t)d * n_nodes + ra.x] - x[(uint64_t)d * n_nodes + rb.x];
        sum_sq += delta * delta;
    }
    err = sqrt(sum_sq) - d_path;                                             // :1273
    rel_sq = (err * err) / (d_path * d_path);                                // :1274
    return true;
}

// ---- fixed-tree reductions ------------------------------------------------------------------------------------------------
// Five 8-byte fields per accumulator; what a field is says how it is combined.
enum FieldOp { SUM_U64, SUM_F64, MAX_F64 };
struct PairFields {                                                        // pairs, sum_rel_sq, max_rel_sq, sum_abs, sum_sq
    static __host__ __device__ constexpr FieldOp op(int f) { return f == 0 ? SUM_U64 : f == 2 ? MAX_F64 : SUM_F64; }
};
struct SortFields {                                                        // steps, abs_err_sum, genomic_sum, sq_err_sum, -
    static __host__ __device__ constexpr FieldOp op(int f) { return f == 3 ? SUM_F64 : SUM_U64; }
};

__device__ __forceinline__ uint64_t combine(const FieldOp op, const uint64_t a, const uint64_t b) {
    if (op == SUM_U64) return a + b;
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return (uint64_t)__double_as_longlong(op == SUM_F64 ? x + y : (y > x ? y : x));
}

// One workgroup's five fields -> partials[field][zi][block].  Butterfly over the wave (both partners of a step compute the
// same commutative a + b), then thread 0 combines the waves in wave order.
template <typename F>
__device__ __forceinline__ void store_block_partials(uint64_t (&v)[5], uint64_t *partials, const uint32_t n_z, const uint32_t zi) {
    __shared__ uint64_t wave_part[Q_BLOCK / 64][5];
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
            v[f] = combine(F::op(f), v[f], (uint64_t)__shfl_xor((unsigned long long)v[f], off, 64));
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int f = 0; f < 5; ++f) wave_part[wave][f] = v[f];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            uint64_t t = wave_part[0][f];
            for (unsigned w = 1; w < Q_BLOCK / 64; ++w) t = combine(F::op(f), t, wave_part[w][f]);
            partials[((uint64_t)f * n_z + zi) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// One item's partials[field][zi][first_block .. first_block + n_blocks) of a row of row_blocks workgroups -> out[0..5), summed in
// workgroup order from zero by thread 0; the others only stage a tile of partials in LDS so that the serial chain runs at LDS
// latency.  One workgroup of Q_BLOCK threads; K7's own launches have first_block = 0 and row_blocks = n_blocks.
template <typename F>
__device__ __forceinline__ void reduce_item_partials(const uint64_t *partials, const uint32_t n_z, const uint32_t zi, const uint32_t row_blocks,
                                                     const uint32_t first_block, const uint32_t n_blocks, uint64_t *out) {
    __shared__ uint64_t tile[5][Q_BLOCK];
    uint64_t acc[5] = {0, 0, 0, 0, 0};                                     // (0 is +0.0 too)
    for (uint32_t base = 0; base < n_blocks; base += Q_BLOCK) {
        const uint32_t n = n_blocks - base < Q_BLOCK ? n_blocks - base : Q_BLOCK;
        if (threadIdx.x < n)
#pragma unroll
            for (int f = 0; f < 5; ++f) tile[f][threadIdx.x] = partials[((uint64_t)f * n_z + zi) * row_blocks + first_block + base + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t b = 0; b < n; ++b)
#pragma unroll
                for (int f = 0; f < 5; ++f) acc[f] = combine(F::op(f), acc[f], tile[f][b]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < 5; ++f) out[f] = acc[f];
}

// ---- K7c and K7k: adjacent steps of every path (measure_layout_quality.rs:130-160) -------------------------------------------
// One thread's pairs (s, s + 1), the thread being threadIdx.x of workgroup `block` of a grid of `blocks` workgroups of Q_BLOCK: s =
// block * Q_BLOCK + threadIdx.x, then in strides of blocks * Q_BLOCK, below n_steps - 1.  spos: the sorted position of every node, by slot.  Reads step_rec[0..n_steps) only.  All integers but sq_sum, which is added in the order of s.
__device__ __forceinline__ void sort_quality_pairs(const uint4 *step_rec, const uint64_t n_steps, const uint64_t *spos, const uint32_t block,
                                                   const uint32_t blocks, uint64_t &steps, uint64_t &abs_sum, uint64_t &gen_sum, double &sq_sum) {
    if (n_steps > 1) {
        const uint64_t n = n_steps - 1, stride = (uint64_t)blocks * Q_BLOCK;
        for (uint64_t s = (uint64_t)block * Q_BLOCK + threadIdx.x; s < n; s += stride) {
            const uint4 ra = step_rec[s], rb = step_rec[s + 1];
            if (rec_path(ra) != rec_path(rb) || ra.x == Q_NO_NODE) continue;               // :139-144
            const uint64_t gd = rec_pos(rb) - rec_pos(ra);                                 // = the first node's length
            const uint64_t pa = spos[ra.x], pb = rb.x == Q_NO_NODE ? 0ull : spos[rb.x];    // :149-150 unwrap_or(0.0)
            const uint64_t ld = pb > pa ? pb - pa : pa - pb;
            const uint64_t ae = ld > gd ? ld - gd : gd - ld;
            ++steps; abs_sum += ae; gen_sum += gd;
            sq_sum += (double)ae * (double)ae;
        }
    }
}

// ---- K7d / K7e / K7f and K7h / K7i / K7j: which paths, pairs and nodes carry the error ------------------------------------
// The per-pair value is pair_error's; a counted pair is STRETCHED when d_layout / d_path > ratio, d_layout = err + d_path.
// The bodies below are what ONE wave does with ONE tile (K7d, K7e), one path (K7d's combine) or one thread with one pair
// (K7f): quality_kernels.hip hands them the tiles of one graph, batch_diagnosis_kernels.hip the LOCAL tiles of every item of a
// batch on the item's own tables — one text, so that an item's rows are its own call's bit for bit.
static constexpr uint32_t Q_NO_PATH = 0xFFFFFFFFu;                       // (a record's path has 31 bits)

struct StretchedPair { uint64_t step_a, step_b, path; double d_path, d_layout; };    // = gfs_stretched_pair

__device__ __forceinline__ bool pair_stretch(const uint4 ra, const uint4 rb, const double *x, const uint64_t n_nodes, const uint32_t dims,
                                             const double ratio, double &err, double &rel_sq, double &d_path, double &d_layout,
                                             bool &stretched) {
    if (!pair_error(ra, rb, x, n_nodes, dims, err, rel_sq)) return false;
    d_path = fabs((double)rec_pos(ra) - (double)rec_pos(rb));              // pair_error's own d_path
    d_layout = err + d_path;
    stretched = d_layout / d_path > ratio;
    return true;
}

// ---- K7d ------------------------------------------------------------------------------------------------------------------
// A step's contribution is five words combined as PairFields combines them: { steps | reverse_steps << 16 | pairs << 32 |
// stretched << 48 (a tile has 512 steps: no counter leaves its 16 bits), sum_rel_sq, max_rel_sq, sum_abs, sum_sq }.
// Per round a segmented inclusive scan over the wave (Hillis-Steele with shuffles, a fixed tree; the steps of a path are
// one run, so "same path at distance off" means the same segment) after lane 0 took over the sum its path carried out of the
// round before.  The lane on a path's LAST step holds the path's sum over the tile: where the path also began inside the
// tile it is the path's result and is written as such; otherwise it is the tile's HEAD partial (the path of the tile's
// first step).  The lane on the tile's last step, where its path goes on, stores the HEAD partial (a path that began at
// or before the tile's first step) or the TAIL partial.  Every partial that K7d's second kernel reads is written by the
// first one in the same call.
__device__ __forceinline__ void store_path_error(uint64_t *out, const uint64_t p, const uint64_t (&cnt)[4], const uint64_t (&v)[5]) {
    uint64_t *o = out + p * 8;                                             // = gfs_path_error
    o[0] = cnt[0]; o[1] = cnt[1]; o[2] = cnt[2];
    o[3] = v[1]; o[4] = v[2]; o[5] = v[3]; o[6] = v[4];
    o[7] = cnt[3];
}
__device__ __forceinline__ void add_tile_counters(uint64_t (&cnt)[4], const uint64_t packed) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] += (packed >> (16 * k)) & 0xFFFFu;
}

// One wave, tile `tile` of a table of n_steps steps: head / tail partials at tile * 5, rows of paths inside the tile at out.
__device__ __forceinline__ void path_tile(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                          const uint32_t dims, const uint64_t z, const double ratio, const uint64_t tile, const unsigned lane,
                                          uint64_t *head, uint64_t *tail, uint64_t *out) {
    const uint64_t lo = tile * Q_TILE, hi = lo + Q_TILE < n_steps ? lo + Q_TILE : n_steps;
    const uint32_t first_path = rec_path(step_rec[lo]);
    const bool head_open = lo > 0 && rec_path(step_rec[lo - 1]) == first_path;     // the first step's path began before the tile
    bool carried = false;
    uint64_t carry[5] = {0, 0, 0, 0, 0};
    for (unsigned r = 0; r < Q_TILE_ROUNDS; ++r) {
        const uint64_t s = lo + (uint64_t)r * 64 + lane;
        uint32_t key = Q_NO_PATH, next = Q_NO_PATH;
        uint64_t v[5] = {0, 0, 0, 0, 0};
        if (s < hi) {
            const uint4 ra = step_rec[s];
            key = rec_path(ra);
            if (s + 1 < n_steps) next = rec_path(step_rec[s + 1]);
            v[0] = 1ull | ((uint64_t)(ra.y >> 31) << 16);
            double err, rel, dp, dl;
            bool st;
            if (z < n_steps && s < n_steps - z && pair_stretch(ra, step_rec[s + z], x, n_nodes, dims, ratio, err, rel, dp, dl, st)) {
                v[0] |= (1ull << 32) | ((uint64_t)st << 48);
                v[1] = (uint64_t)__double_as_longlong(rel); v[2] = v[1];
                v[3] = (uint64_t)__double_as_longlong(fabs(err)); v[4] = (uint64_t)__double_as_longlong(err * err);
            }
        }
        if (lane == 0 && carried)
#pragma unroll
            for (int f = 0; f < 5; ++f) v[f] = combine(PairFields::op(f), carry[f], v[f]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t ku = (uint32_t)__shfl_up((int)key, off, 64);
            const bool take = lane >= (unsigned)off && ku == key;
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v[f], off, 64);
                if (take) v[f] = combine(PairFields::op(f), u, v[f]);
            }
        }
        if (s < hi) {
            if (next != key) {                                          // the path's last step
                if (key == first_path && head_open) {
#pragma unroll
                    for (int f = 0; f < 5; ++f) head[tile * 5 + f] = v[f];
                } else {
                    uint64_t cnt[4] = {0, 0, 0, 0};
                    add_tile_counters(cnt, v[0]);
                    store_path_error(out, key, cnt, v);
                }
            } else if (s + 1 == hi) {                                   // the tile's last step, the path goes on
                uint64_t *part = key == first_path ? head : tail;
#pragma unroll
                for (int f = 0; f < 5; ++f) part[tile * 5 + f] = v[f];
            }
        }
        // lane 63's path goes on in the next round (all lanes agree: the values are lane 63's)
        carried = __shfl((int)(s < hi && next == key), 63, 64) != 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) carry[f] = (uint64_t)__shfl((unsigned long long)v[f], 63, 64);
    }
}

// One wave, path p of a table whose record is pr = { first step lo, steps, -, first step hi }: the partials of the tiles the
// path crosses, folded IN TILE ORDER (64 tiles are loaded at a time, one per lane, and taken in lane order; every lane folds
// the same values).  A path inside one tile was written by the tile pass and is left alone; a path without steps gets zeros.
__device__ __forceinline__ void path_fold(const uint4 pr, const uint64_t p, const unsigned lane, const uint64_t *head, const uint64_t *tail,
                                          uint64_t *out) {
    const uint64_t b = (uint64_t)pr.x | ((uint64_t)pr.w << 32), cnt = pr.y;
    uint64_t acc[5] = {0, 0, 0, 0, 0}, counters[4] = {0, 0, 0, 0};      // (16 bits hold a tile's counters, not a path's)
    if (cnt) {
        const uint64_t tb = b / Q_TILE, te = (b + cnt - 1) / Q_TILE;
        if (tb == te) return;
        for (uint64_t base = tb; base <= te; base += 64) {
            const uint64_t t = base + lane;
            const unsigned n = te - base + 1 < 64 ? (unsigned)(te - base + 1) : 64u;
            uint64_t v[5] = {0, 0, 0, 0, 0};
            if (t <= te) {
                const uint64_t *part = (t == tb && b % Q_TILE != 0) ? tail : head;
#pragma unroll
                for (int f = 0; f < 5; ++f) v[f] = part[t * 5 + f];
            }
            for (unsigned l = 0; l < n; ++l) {
                add_tile_counters(counters, (uint64_t)__shfl((unsigned long long)v[0], (int)l, 64));
#pragma unroll
                for (int f = 1; f < 5; ++f)
                    acc[f] = combine(PairFields::op(f), acc[f], (uint64_t)__shfl((unsigned long long)v[f], (int)l, 64));
            }
        }
    }
    if (lane == 0) store_path_error(out, p, counters, acc);
}

// ---- K7e ------------------------------------------------------------------------------------------------------------------
// One wave, tile `tile`: its stretched pairs are counted (ballots); with a list, pair number at + (stretched pairs before it
// in the tile) is written where that is < cap.  Returns `at` advanced by the tile's stretched pairs (all lanes agree).
__device__ __forceinline__ uint64_t stretched_tile(const uint4 *step_rec, const uint64_t n_steps, const double *x, const uint64_t n_nodes,
                                                   const uint32_t dims, const uint64_t z, const double ratio, const uint64_t tile,
                                                   const unsigned lane, uint64_t at, StretchedPair *list, const uint64_t cap) {
    const uint64_t lo = tile * Q_TILE, hi = lo + Q_TILE < n_steps ? lo + Q_TILE : n_steps;
    for (unsigned r = 0; r < Q_TILE_ROUNDS; ++r) {
        const uint64_t s = lo + (uint64_t)r * 64 + lane;
        double err, rel, dp = 0.0, dl = 0.0;
        bool st = false;
        uint4 ra = make_uint4(0, 0, 0, 0);
        if (s < hi && z < n_steps && s < n_steps - z) {
            ra = step_rec[s];
            if (!pair_stretch(ra, step_rec[s + z], x, n_nodes, dims, ratio, err, rel, dp, dl, st)) st = false;
        }
        const unsigned long long m = __ballot(st);
        if (list && st) {
            const uint64_t k = at + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (k < cap) list[k] = StretchedPair{s, s + z, (uint64_t)rec_path(ra), dp, dl};
        }
        at += (uint64_t)__popcll(m);
    }
    return at;
}

// ---- K7f ------------------------------------------------------------------------------------------------------------------
// One thread, a counted pair (ra, rb) of relative error rel_sq.  Per node SLOT: pairs and stretched pairs that touch the node
// (integer atomic adds; a pair from a node to itself counts once) and the largest rel_sq (unsigned 64-bit atomic max on the
// bits of the non-negative double: same order as the values).  Sums of integers and a maximum do not depend on the order of
// arrival.  The maximum only grows, so a plain load that already shows a value >= ours, however stale, makes the atomic
// unnecessary.
__device__ __forceinline__ void node_pair(const uint4 ra, const uint4 rb, const double rel_sq, const bool st, unsigned long long *pairs,
                                          unsigned long long *stretched, unsigned long long *max_bits) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(rel_sq);
    const uint32_t ends[2] = {ra.x, rb.x};
    for (int k = 0; k < (ra.x == rb.x ? 1 : 2); ++k) {
        const uint32_t slot = ends[k];
        atomicAdd(&pairs[slot], 1ull);
        if (st) atomicAdd(&stretched[slot], 1ull);
        if (max_bits[slot] < bits) atomicMax(&max_bits[slot], bits);
    }
}

}  // namespace gfs
