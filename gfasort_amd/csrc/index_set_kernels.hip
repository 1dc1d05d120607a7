// index_set_kernels.hip — K3b: THE index build — the internal node layout, and K3, PathIndex::from_graph (src/sgd.rs:34-71): step
// positions = per-path exclusive prefix sum of node lengths over the steps, written straight into the 16-byte step records — of
// one graph or of MANY in one pass.  The items of a set are one disjoint graph, the UNION (index_set.h): one scan over all steps,
// two radix sorts over all nodes, the pointer-jumping fixpoints once over all nodes (rocPRIM for the scan and the sorts; the kernels
// around them are hand-written).  The kernels look an element's item up in the item table (a binary search: the table is small and
// stays in cache) and REBASE on the way out — slot = union rank - the item's first node, path id = union path - the item's first
// path, positions from scan differences — so that every item's arrays in the arena hold the bits a context of that graph alone
// holds.  gfs_ctx_create builds its context here too, as a union of one item: the look-up runs no iteration, every rebase
// subtracts 0.  Integer arithmetic throughout.
//
// ---- internal node layout (first-visit path order with branches placed where they branch off) -----------------------
// Base rule: nodes in the order the paths first step on them, nodes no path visits last in index order (min-reduction over
// the steps + stable sort, so that a 4.5e9-step graph takes 0.3 s instead of 25 s on one host core).  The same pass
// validates step_node (dense index < n_nodes, or NO_NODE).
// Refinement: the first visits of a path come in RUNS of consecutive steps.  A run that starts its path is a ROOT run and
// keeps its place.  Any other run BRANCHES OFF the node its path stepped on just before it (its anchor) — an alternative
// allele of a bubble, first seen by the 7th haplotype, branches off the node before the bubble — and is placed right after
// the root-run node its chain of anchors leads to, instead of where the 7th haplotype happens to come in step order.
// sort key of node v = 4*(first[v] + 1) for a root-run node, 4*(first[root(v)] + 1) + 1 otherwise (any keys of that order do:
// 2*first and 2*first + 1 for one graph); ties (branches of one root node) in first-visit order.  Why: a run of 64 consecutive
// path steps then touches neighbouring position words on a bubble graph too, not 8 lines of main chain plus a scattered line per
// alternative allele (bubble graphs of 0.5M / 2M nodes: 63.9 -> 77.6 and 68.2 -> 79.7 G updates/s,
// profiles/r02/relayout_probe.log; chains and window graphs are unchanged — they have no branches).  gfs_shared_node_layout
// (multi.hip) is the same rule on the host.
//
// Where the union differs from one graph:
//   * a node no path visits goes last WITHIN ITS ITEM: the sort keys are 4*(first + 1) (+ 1 for a branch) for a visited node and
//     4*(the item's last step + 1) + 2 for an unvisited one — above every key of its item, below every key of the next; first
//     visits are union steps, so visited nodes come item by item anyway, and the stable sorts keep equal keys (unvisited nodes of
//     an item, and of step-less items behind it) in union order, which is item order, then index order;
//   * an item's first step is the first step of a path of the union's path table, so the look at step f - 1 and the 64-step window
//     of `rep`, which stop at path starts, never cross into the item before;
//   * the bad-step flag is the lowest bad item.
#include "index_set.h"
#include "device_memory.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>
#include <type_traits>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace gfs {

constexpr uint32_t NO_NODE_U32 = 0xFFFFFFFFu;
constexpr unsigned KEY_BITS = 43;                 // 4 * (2^40 + 1) + 2 < 2^43
constexpr int JUMP_ROUNDS = 40, JUMP_CHUNK = 4;    // rounds of a fixpoint (31 suffice for 2^31 nodes); rounds per read-back

// last i with items[i].*off <= v (items of no nodes / steps / paths share a boundary with the next one: take the last, which is
// the one v lies in); items[n_items].*off is the total, above every v
__host__ __device__ __forceinline__ uint32_t item_of(const SetItem *items, uint32_t n_items, uint64_t v, uint64_t SetItem::*off) {
    uint32_t lo = 0, hi = n_items;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (items[mid].*off <= v) lo = mid; else hi = mid; }
    return lo;
}
// path of union step s: last p with path_first[p] <= s (empty paths share a boundary: take the last)
__host__ __device__ __forceinline__ uint32_t path_of(const uint64_t *path_first, uint32_t n_paths, uint64_t s) {
    uint32_t lo = 0, hi = n_paths;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (path_first[mid] <= s) lo = mid; else hi = mid; }
    return lo;
}
__device__ __forceinline__ bool set_is_path_start(const uint64_t *path_first, uint32_t n_paths, uint64_t s) {
    uint32_t lo = 0, hi = n_paths;                                         // first path whose first step is >= s
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (path_first[mid] < s) lo = mid + 1; else hi = mid; }
    return lo < n_paths && path_first[lo] == s;
}
__device__ __forceinline__ uint32_t set_ceil_log2(uint32_t v) { return v <= 1 ? 0u : 32u - (uint32_t)__clz((int)(v - 1)); }
__device__ __forceinline__ unsigned long long unvisited_key(const SetItem *items, uint32_t i) { return 4ull * items[i + 1].step_off + 2ull; }

// ---- node layout ---------------------------------------------------------------------------------------------------------------
// first[v] = first union step on union node v; *bad = lowest item with a step naming a node it does not have
__global__ void set_first_visit_kernel(SetUnion u, unsigned long long *first, uint32_t *bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < u.n_steps; s += stride) {
        const uint32_t n = u.step_node[s];
        if (n == NO_NODE_U32) continue;
        const uint32_t i = item_of(u.items, u.n_items, s, &SetItem::step_off);
        const uint64_t base = u.items[i].node_off;
        if (n >= u.items[i + 1].node_off - base) { atomicMin(bad, i); continue; }
        if (first[base + n] > s) atomicMin(&first[base + n], (unsigned long long)s);   // the plain read only skips work
    }
}
// the key of the first sort (first-visit order, unvisited nodes last within their item) and the ids it carries
__global__ void set_first_key_kernel(SetUnion u, const unsigned long long *first, unsigned long long *key, uint32_t *ids) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < u.n_nodes; v += stride) {
        const unsigned long long f = first[v];
        key[v] = f == ~0ull ? unvisited_key(u.items, item_of(u.items, u.n_items, v, &SetItem::node_off)) : 4ull * (f + 1ull);
        ids[v] = (uint32_t)v;
    }
}
// up[v] = v for the first node of a run of first visits (and for unvisited nodes), else the node visited just before it
__global__ void set_run_up_kernel(SetUnion u, const unsigned long long *first, uint32_t *up) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < u.n_nodes; v += stride) {
        const unsigned long long f = first[v];
        uint32_t w = (uint32_t)v;
        if (f != ~0ull && !set_is_path_start(u.path_first, (uint32_t)u.n_paths, f)) {   // (step 0 and every item's first step start a path)
            const uint32_t p = u.step_node[f - 1];                                      // same path, so the same item as v
            if (p != NO_NODE_U32) {
                const uint64_t q = u.items[item_of(u.items, u.n_items, v, &SetItem::node_off)].node_off + p;
                if (first[q] == f - 1) w = (uint32_t)q;                                 // the previous step was a first visit too
            }
        }
        up[v] = w;
    }
}
// pointer jumping: out[v] = in[in[v]]
__global__ void set_jump_kernel(const uint32_t *in, uint32_t *out, uint64_t n_nodes, uint32_t *changed) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += stride) {
        const uint32_t a = in[v], b = in[a];
        out[v] = b;
        if (b != a) *changed = 1;
    }
}
// anc[v] = v for a node of a root run (and unvisited nodes), else the node its run branches off; head[v] = first node of v's run
__global__ void set_anchor_kernel(SetUnion u, const unsigned long long *first, const uint32_t *head, uint32_t *anc) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < u.n_nodes; v += stride) {
        uint32_t a = (uint32_t)v;
        if (first[v] != ~0ull) {
            const unsigned long long fh = first[head[v]];
            if (!set_is_path_start(u.path_first, (uint32_t)u.n_paths, fh)) {
                const uint32_t p = u.step_node[fh - 1];
                if (p != NO_NODE_U32) a = (uint32_t)(u.items[item_of(u.items, u.n_items, v, &SetItem::node_off)].node_off + p);
            }
        }
        anc[v] = a;
    }
}
// keys in first-visit order: key[r] for the node ids_by_first[r]
__global__ void set_branch_key_kernel(SetUnion u, const unsigned long long *first, const uint32_t *root, const uint32_t *ids_by_first,
                                      unsigned long long *key) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < u.n_nodes; r += stride) {
        const uint32_t v = ids_by_first[r];
        const unsigned long long f = first[v];
        const uint32_t t = root[v];
        key[r] = f == ~0ull ? unvisited_key(u.items, item_of(u.items, u.n_items, v, &SetItem::node_off))
                            : (t == v ? 4ull * (f + 1ull) : 4ull * (first[t] + 1ull) + 1ull);
    }
}
// the item's own layout: slot of its dense node = union rank - its first node (an item's nodes hold the ranks of its own range:
// the keys are grouped by item)
__global__ void set_scatter_rank_kernel(SetUnion u, const uint32_t *sorted_node) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < u.n_nodes; r += stride) {
        const uint64_t v = sorted_node[r];
        const SetItem it = u.items[item_of(u.items, u.n_items, v, &SetItem::node_off)];
        reinterpret_cast<uint32_t *>(u.arena + it.perm)[v - it.node_off] = (uint32_t)(r - it.node_off);
    }
}

// ---- K3 over the union ---------------------------------------------------------------------------------------------------------
// len(s) = sequence length of the step's node (0 for an absent node, sgd.rs:52-54); len(n_steps) = 0.  Fed to the scan through a
// transform iterator, so the lengths are never materialised (8 B per step less scratch).
struct SetStepLen {
    SetUnion u;
    __host__ __device__ uint64_t operator()(uint64_t s) const {
        if (s >= u.n_steps) return 0;
        const uint32_t n = u.step_node[s];
        if (n == NO_NODE_U32) return 0ull;
        const SetItem &it = u.items[item_of(u.items, u.n_items, s, &SetItem::step_off)];
        return (uint64_t)reinterpret_cast<const uint32_t *>(u.arena + it.nlen)[n];
    }
};
// Crowding statistics of the nodes (sgd_device.h crowd_shift), by union node: cnt[v] = steps on node v; rep[v] = the most visits
// to v within any 64 consecutive steps of one path (a step counts its node's earlier visits among the 63 steps before it, not
// looking across the start of its path).
__global__ void set_node_stats_kernel(SetUnion u, uint32_t *cnt, uint32_t *rep) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < u.n_steps; s += stride) {
        const uint32_t n = u.step_node[s];
        if (n == NO_NODE_U32) continue;
        const uint64_t v = u.items[item_of(u.items, u.n_items, s, &SetItem::step_off)].node_off + n;
        atomicAdd(&cnt[v], 1u);
        const uint64_t begin = u.path_first[path_of(u.path_first, (uint32_t)u.n_paths, s)], from = s - begin > 63 ? s - 63 : begin;
        uint32_t c = 1;
        for (uint64_t t = from; t < s; ++t) c += u.step_node[t] == n;      // (one path, one item: its own indices compare)
        if (c > 1 && rep[v] < c) atomicMax(&rep[v], c);
    }
}
// rec[s] = { internal node slot | NO_NODE, path | rev<<31, pos lo, pos hi (23 bits) | a<<23 | b<<29 } with pos = scan[s] -
// scan[first(path)], the slot and the path id the item's own, into the item's array.  u.trip (a union of one item): trip[s] =
// { rec.x, rec.z } as well.  facts (nullable): [0] = the largest pos, [1] / [2] = the largest a / b written, one atomic each per wave.
__global__ void set_fill_records_kernel(SetUnion u, const uint64_t *scan, const uint32_t *cnt, const uint32_t *rep, unsigned long long *facts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long max_pos = 0, max_a = 0, max_b = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < u.n_steps; s += stride) {
        const uint32_t p = path_of(u.path_first, (uint32_t)u.n_paths, s);
        const SetItem it = u.items[item_of(u.items, u.n_items, s, &SetItem::step_off)];   // (= the item of path p)
        const uint64_t pos = scan[s] - scan[u.path_first[p]];
        const uint32_t n = u.step_node[s];
        uint4 r;
        r.x = n == NO_NODE_U32 ? NO_NODE_U32 : reinterpret_cast<const uint32_t *>(u.arena + it.perm)[n];
        uint32_t crowd = 0;
        if (n != NO_NODE_U32) {
            const uint32_t a = set_ceil_log2(cnt[it.node_off + n]), b = set_ceil_log2(rep[it.node_off + n]);
            crowd = ((a > 63u ? 63u : a) << 23) | ((b > 7u ? 7u : b) << 29);
            if (a > max_a) max_a = a;
            if (b > max_b) max_b = b;
        }
        if (pos > max_pos) max_pos = pos;
        r.y = (uint32_t)(p - it.path_off) | ((uint32_t)(u.step_is_rev[s] & 1) << 31);
        r.z = (uint32_t)pos; r.w = ((uint32_t)(pos >> 32) & 0x7FFFFFu) | crowd;
        reinterpret_cast<uint4 *>(u.arena + it.rec)[s - it.step_off] = r;
        if (u.trip) u.trip[s] = make_uint2(r.x, r.z);                      // (one item: s is its own step)
    }
    if (!facts) return;
    for (int off = 32; off > 0; off >>= 1) {                               // (every lane arrives here: SET_BLOCK is whole waves)
        const unsigned long long p = __shfl_xor(max_pos, off, 64), a = __shfl_xor(max_a, off, 64), b = __shfl_xor(max_b, off, 64);
        max_pos = p > max_pos ? p : max_pos; max_a = a > max_a ? a : max_a; max_b = b > max_b ? b : max_b;
    }
    if ((threadIdx.x & 63) == 0) {
        if (max_pos) atomicMax(&facts[0], max_pos);
        if (max_a) atomicMax(&facts[1], max_a);
        if (max_b) atomicMax(&facts[2], max_b);
    }
}
// t < n_paths: path t's record { first step lo, steps, 2^32 mod steps, first step hi } in its item's numbering and its length in
// bp (scan == nullptr: no steps anywhere, every length 0); t - n_paths = an item: its zeroed padding record
__global__ void set_paths_kernel(SetUnion u, const uint64_t *scan) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, total = u.n_paths + u.n_items;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t >= u.n_paths) {
            const uint32_t i = (uint32_t)(t - u.n_paths);
            reinterpret_cast<uint4 *>(u.arena + u.items[i].rec)[u.items[i + 1].step_off - u.items[i].step_off] = make_uint4(0, 0, 0, 0);
            if (u.trip) u.trip[u.n_steps] = make_uint2(0, 0);
            continue;
        }
        const SetItem it = u.items[item_of(u.items, u.n_items, t, &SetItem::path_off)];
        const uint64_t fb = u.path_first[t], fe = u.path_first[t + 1], b = fb - it.step_off;
        const uint32_t c = (uint32_t)(fe - fb);
        reinterpret_cast<uint4 *>(u.arena + it.prec)[t - it.path_off] = make_uint4((uint32_t)b, c, c ? (uint32_t)(0u - c) % c : 0u, (uint32_t)(b >> 32));
        reinterpret_cast<uint64_t *>(u.arena + it.plen)[t - it.path_off] = scan ? scan[fe] - scan[fb] : 0ull;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
namespace {
// the pieces of the scratch, every piece 256-byte aligned; `bytes` is their sum
struct Work {
    unsigned long long *first, *key_a, *key_b;
    uint32_t *ids_a, *ids_b, *a, *b, *cnt, *rep;
    uint64_t *scan;
    uint32_t *flags;                                                       // [0]: lowest bad item; [1 + round]: a fixpoint round changed something
    unsigned long long *facts;                                             // [3]: largest position, a and b of the records (set_fill_records_kernel)
    void *tmp;
    size_t tmp_bytes;
    uint64_t cnt_rep_bytes, bytes;                                         // (cnt and rep are adjacent: one memset zeroes both)
};
hipError_t plan_work(uint64_t N, uint64_t S, void *d_work, Work &w) {
    size_t sort_tmp = 0, scan_tmp = 0;
    hipError_t e = hipSuccess;
    if (N) e = rocprim::radix_sort_pairs(nullptr, sort_tmp, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                         (size_t)N, 0, KEY_BITS, 0);
    if (e != hipSuccess) return e;
    if (S) {
        auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), SetStepLen{SetUnion{}});
        e = rocprim::exclusive_scan(nullptr, scan_tmp, lens, (uint64_t *)nullptr, (uint64_t)0, (size_t)(S + 1), rocprim::plus<uint64_t>(), 0);
        if (e != hipSuccess) return e;
    }
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_work);            // (null where only the size is asked for)
    uint64_t at = 0;
    auto take = [&at, base](auto *&piece, uint64_t bytes) {
        piece = reinterpret_cast<std::remove_reference_t<decltype(piece)>>(base + at);
        at += round256(bytes ? bytes : 1);
    };
    take(w.first, N * 8); take(w.key_a, N * 8); take(w.key_b, N * 8);
    take(w.ids_a, N * 4); take(w.ids_b, N * 4); take(w.a, N * 4); take(w.b, N * 4);
    take(w.cnt, N * 4); take(w.rep, N * 4);
    w.cnt_rep_bytes = round256(N ? N * 4 : 1) + N * 4;
    take(w.scan, S ? (S + 1) * 8 : 0);
    take(w.flags, (1 + 2 * JUMP_ROUNDS) * sizeof(uint32_t));
    take(w.facts, 3 * sizeof(unsigned long long));
    w.tmp_bytes = std::max(sort_tmp, scan_tmp);
    take(w.tmp, w.tmp_bytes);
    w.bytes = at;
    return hipSuccess;
}
const dim3 over_steps(SET_STEP_BLOCKS), over_nodes(SET_NODE_BLOCKS), block(SET_BLOCK);
}  // namespace

hipError_t index_set_work_bytes(uint64_t n_nodes, uint64_t n_steps, uint64_t *bytes) {
    Work w{};
    const hipError_t e = plan_work(n_nodes, n_steps, nullptr, w);
    *bytes = w.bytes;
    return e;
}

hipError_t index_set_layout_device(const SetUnion &u, void *d_work, bool layout_given, uint32_t *bad_item, uint64_t *launches) {
    *bad_item = SET_NO_BAD_ITEM;
    const uint64_t N = u.n_nodes, S = u.n_steps;
    Work w{};
    hipError_t e = plan_work(N, S, d_work, w);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.flags, 0xFF, sizeof(uint32_t), 0)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.flags + 1, 0, 2 * JUMP_ROUNDS * sizeof(uint32_t), 0)) != hipSuccess) return e;
    *launches += 2;
    if (N) {
        if ((e = hipMemsetAsync(w.first, 0xFF, N * 8, 0)) != hipSuccess) return e;
        ++*launches;
    }
    if (S) {
        hipLaunchKernelGGL(set_first_visit_kernel, over_steps, block, 0, 0, u, w.first, w.flags);
        ++*launches;
        // the one read-back the build cannot do without: the kernels below, and K3, index by step_node
        if ((e = hipMemcpy(bad_item, w.flags, sizeof(uint32_t), hipMemcpyDeviceToHost)) != hipSuccess) return e;
        if (*bad_item != SET_NO_BAD_ITEM) return hipSuccess;
    }
    if (!N || layout_given) return hipGetLastError();
    hipLaunchKernelGGL(set_first_key_kernel, over_nodes, block, 0, 0, u, w.first, w.key_a, w.ids_a);
    e = rocprim::radix_sort_pairs(w.tmp, w.tmp_bytes, (uint64_t *)w.key_a, (uint64_t *)w.key_b, w.ids_a, w.ids_b, (size_t)N, 0, KEY_BITS, 0);
    *launches += 2;
    if (e != hipSuccess) return e;
    uint32_t *d_ids = w.ids_b, *d_ids_other = w.ids_a;                     // ids in first-visit order (stable: unvisited nodes in index order)
    if (S) {
        // branches: run heads by pointer jumping along the runs, anchors, roots by pointer jumping along the anchors.  A round past
        // the fixpoint changes nothing, so the rounds go out JUMP_CHUNK at a time and their flags come back in one copy.
        uint32_t *d_a = w.a, *d_b = w.b;
        auto jump_to_fixpoint = [&](uint32_t *&cur, uint32_t *&other, uint32_t *flags) -> hipError_t {
            for (int round = 0; round < JUMP_ROUNDS; round += JUMP_CHUNK) {
                for (int k = 0; k < JUMP_CHUNK; ++k) {
                    hipLaunchKernelGGL(set_jump_kernel, over_nodes, block, 0, 0, cur, other, N, flags + round + k);
                    std::swap(cur, other);
                }
                *launches += JUMP_CHUNK;
                uint32_t changed[JUMP_CHUNK];
                const hipError_t err = hipMemcpy(changed, flags + round, sizeof changed, hipMemcpyDeviceToHost);
                if (err != hipSuccess) return err;
                if (std::find(changed, changed + JUMP_CHUNK, 0u) != changed + JUMP_CHUNK) break;
            }
            return hipSuccess;
        };
        hipLaunchKernelGGL(set_run_up_kernel, over_nodes, block, 0, 0, u, w.first, d_a);
        ++*launches;
        if ((e = jump_to_fixpoint(d_a, d_b, w.flags + 1)) != hipSuccess) return e;                  // d_a = run head of every node
        hipLaunchKernelGGL(set_anchor_kernel, over_nodes, block, 0, 0, u, w.first, d_a, d_b);
        std::swap(d_a, d_b);
        ++*launches;
        if ((e = jump_to_fixpoint(d_a, d_b, w.flags + 1 + JUMP_ROUNDS)) != hipSuccess) return e;    // d_a = root of every node
        hipLaunchKernelGGL(set_branch_key_kernel, over_nodes, block, 0, 0, u, w.first, d_a, d_ids, w.key_a);
        // stable sort by key of the ids already in first-visit order: (key, first visit)
        e = rocprim::radix_sort_pairs(w.tmp, w.tmp_bytes, (uint64_t *)w.key_a, (uint64_t *)w.key_b, d_ids, d_ids_other, (size_t)N, 0, KEY_BITS, 0);
        *launches += 2;
        if (e != hipSuccess) return e;
        std::swap(d_ids, d_ids_other);
    }
    hipLaunchKernelGGL(set_scatter_rank_kernel, over_nodes, block, 0, 0, u, d_ids);
    ++*launches;
    return hipGetLastError();
}

hipError_t index_set_records_device(const SetUnion &u, void *d_work, uint64_t *launches, RecordFacts *facts) {
    const uint64_t N = u.n_nodes, S = u.n_steps;
    Work w{};
    hipError_t e = plan_work(N, S, d_work, w);
    if (e != hipSuccess) return e;
    if (S) {
        auto lens = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), SetStepLen{u});
        e = rocprim::exclusive_scan(w.tmp, w.tmp_bytes, lens, w.scan, (uint64_t)0, (size_t)(S + 1), rocprim::plus<uint64_t>(), 0);
        if (e != hipSuccess) return e;
        if ((e = hipMemsetAsync(w.cnt, 0, w.cnt_rep_bytes, 0)) != hipSuccess) return e;
        hipLaunchKernelGGL(set_node_stats_kernel, over_steps, block, 0, 0, u, w.cnt, w.rep);
        if (facts) {
            if ((e = hipMemsetAsync(w.facts, 0, 3 * sizeof(unsigned long long), 0)) != hipSuccess) return e;
            ++*launches;
        }
        hipLaunchKernelGGL(set_fill_records_kernel, over_steps, block, 0, 0, u, w.scan, w.cnt, w.rep, facts ? w.facts : (unsigned long long *)nullptr);
        *launches += 4;
    }
    hipLaunchKernelGGL(set_paths_kernel, dim3(SET_PATH_BLOCKS), block, 0, 0, u, S ? w.scan : (const uint64_t *)nullptr);
    ++*launches;
    if (facts) {
        unsigned long long h[3] = {0, 0, 0};
        if (S && (e = hipMemcpy(h, w.facts, sizeof h, hipMemcpyDeviceToHost)) != hipSuccess) return e;
        facts->max_pos = h[0]; facts->max_a = (uint32_t)h[1]; facts->max_b = (uint32_t)h[2];
    }
    return hipGetLastError();
}

// loads this translation unit's code object (HIP loads modules on first use); see gfs_warmup
hipError_t warm_module_index_set() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&set_paths_kernel));
}

}  // namespace gfs
