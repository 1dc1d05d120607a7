// index_set_plan.h — where things lie in an index build (K3b), host arithmetic only: the five index arrays of every item in the
// arena (gfs_ctx_set_plan), and the input head in front of the build's scratch.  Plain C++, so that a test compiles it alone.
#pragma once
#include <stdint.h>

namespace gfs {

constexpr uint64_t round256(uint64_t b) { return (b + 255ull) & ~255ull; }
constexpr int SET_KINDS = 5;                       // step_rec, path_rec, path_len, perm, node_len
constexpr uint64_t SET_ITEM_BYTES = 64;            // sizeof(SetItem) (index_set.h)

inline uint64_t set_kind_bytes(int kind, uint64_t N, uint64_t S, uint64_t P) {
    switch (kind) {
    case 0: return (S + 1) * 16;                   // (one record of padding: the layout team kernels read the record AFTER a step)
    case 1: return (P ? P : 1) * 16;
    case 2: return (P ? P : 1) * 8;
    default: return (N ? N : 1) * 4;               // perm, node_len
    }
}
// offsets[SET_KINDS * i + kind]: by kind, then by item, every array 256-byte aligned — the node lengths of all items (and their
// layouts) are one range of the arena, one copy each.  Returns the arena's bytes.
inline uint64_t set_arena_plan(const uint64_t *n_nodes, const uint64_t *n_steps, const uint64_t *n_paths, uint64_t n, uint64_t *offsets) {
    uint64_t at = 0;
    for (int kind = 0; kind < SET_KINDS; ++kind)
        for (uint64_t i = 0; i < n; ++i) {
            offsets[SET_KINDS * i + kind] = at;
            at += round256(set_kind_bytes(kind, n_nodes[i], n_steps[i], n_paths[i]));
        }
    return at;
}

// The inputs of a build, at the head of its scratch: [step_node | path_first | item table | step_is_rev], each 256-byte aligned;
// the build's own scratch (index_set_work_bytes) starts at `bytes`.
struct SetInputHead {
    uint64_t at_first, at_items, at_rev, bytes;
};
inline SetInputHead set_input_head(uint64_t S, uint64_t P, uint64_t n) {
    SetInputHead h{};
    h.at_first = round256(S * 4);
    h.at_items = h.at_first + round256((P + 1) * 8);
    h.at_rev = h.at_items + round256((n + 1) * SET_ITEM_BYTES);
    h.bytes = h.at_rev + round256(S);
    return h;
}

}  // namespace gfs
