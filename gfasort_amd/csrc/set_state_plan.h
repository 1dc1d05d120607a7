// set_state_plan.h — where things lie in a set setup (gfs_ctx_set_setup_*, capi_set.hip), host arithmetic only: the state arrays
// of every item in the set's state arena (gfs_ctx_set_state_plan), and the zeta tables that items of like parameters share.
// Plain C++ against the public header, so that a test compiles it alone (host_tables.hip beside it for gfs_zeta_table).
#pragma once
#include "../../include/gfasort_hip.h"
#include "index_set_plan.h"                        // round256

#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace gfs {

// The state arrays of a set-up context, in the order they lie in the arena (GFS_STATE_* of the public header).  The first five are
// zeroed by a setup and lie in front: ONE memset covers them.  The RNG words are written by the seeding kernel.  The last two come
// from the host and lie at the end, the seeding kernel's tables behind them: ONE copy from the staging buffer covers all three.
constexpr int SET_STATE_KINDS = GFS_STATE_KINDS;
static_assert(GFS_STATE_POSITIONS == 0 && GFS_STATE_TRACE_COUNTS == 4 && GFS_STATE_RNG == 5 && GFS_STATE_ZETAS == 6 &&
              GFS_STATE_SCHEDULE == 7 && GFS_STATE_KINDS == 8, "zeroed kinds first, uploaded kinds last");

// offsets[SET_STATE_KINDS * i + kind] for bytes[SET_STATE_KINDS * i + kind]: by kind, then by item, every array 256-byte aligned;
// an array of 0 bytes takes no room (its offset is the next array's).  Returns the arena's bytes, the end of the last array's room.
inline uint64_t set_state_plan(const uint64_t *bytes, uint64_t n, uint64_t *offsets) {
    uint64_t at = 0;
    for (int kind = 0; kind < SET_STATE_KINDS; ++kind)
        for (uint64_t i = 0; i < n; ++i) {
            offsets[SET_STATE_KINDS * i + kind] = at;
            at += round256(bytes[SET_STATE_KINDS * i + kind]);
        }
    return at;
}
// where a kind's arrays begin (n >= 1): the zeroed range is [0, begin of RNG), the uploaded one [begin of ZETAS, arena_bytes)
inline uint64_t set_state_kind_begin(const uint64_t *offsets, int kind) { return offsets[kind]; }

// ---- zeta tables ---------------------------------------------------------------------------------------------------------------
// A setup sums the zeta table (sgd.rs:317-331) only as far as its kernels read it: to the space that feeds the last staged index
// (zlen_staged - 1), never beyond the caller's.  The table of those clamped parameters, zero-padded to the full length, is what
// goes to the device.
inline uint64_t zeta_clamped_space(const gfs_sgd_params &p, uint64_t zlen_staged) {
    const uint64_t m = zlen_staged - 1;                                    // last staged index
    const uint64_t need_i = m <= p.space_max ? m : p.space_max + (m - p.space_max - 1) * p.space_quantization_step;
    return std::min<uint64_t>(p.space, std::max<uint64_t>(need_i, 1));
}

// zetas[i] depends on theta, space_max and space_quantization_step, and on space only through where the table ends: the table of
// a smaller space is a PREFIX of the table of a larger one (entry k <= space_max is the running sum at k, entry space_max + 1 + j
// the running sum at space_max + j * step, and gfs_zeta_table_len admits exactly the entries whose sum stops at or before space).
// So items that share the three get slices of one table, summed once to the largest space any of them needs — in the reference's
// order, so that a slice is bit for bit the item's own table.
struct SharedZetaTables {
    std::vector<std::vector<double>> tables;       // one per distinct (theta, space_max, step)
    std::vector<uint32_t> table_of;                // per item; unused for an item with `needed[i]` false
};
inline bool zeta_same_key(const gfs_sgd_params &a, const gfs_sgd_params &b) {
    return memcmp(&a.theta, &b.theta, sizeof a.theta) == 0 && a.space_max == b.space_max && a.space_quantization_step == b.space_quantization_step;
}
// clamped[i]: item i's parameters with space = zeta_clamped_space; needed[i] (nullable: all): whether item i has a table at all
inline SharedZetaTables shared_zeta_tables(const gfs_sgd_params *clamped, const uint8_t *needed, uint64_t n) {
    SharedZetaTables out;
    out.table_of.assign(n, 0);
    std::vector<gfs_sgd_params> widest;            // per table: the parameters of the item with the largest space
    for (uint64_t i = 0; i < n; ++i) {
        if (needed && !needed[i]) continue;
        size_t t = 0;
        while (t < widest.size() && !zeta_same_key(widest[t], clamped[i])) ++t;
        if (t == widest.size()) widest.push_back(clamped[i]);
        else if (clamped[i].space > widest[t].space) widest[t].space = clamped[i].space;
        out.table_of[i] = (uint32_t)t;
    }
    out.tables.resize(widest.size());
    for (size_t t = 0; t < widest.size(); ++t) {
        out.tables[t].assign(gfs_zeta_table_len(&widest[t]), 0.0);
        gfs_zeta_table(&widest[t], out.tables[t].data());
    }
    return out;
}
// item's table into out[zlen_full], which the caller has zeroed: the first gfs_zeta_table_len(clamped) entries of the shared one
inline void zeta_slice(const std::vector<double> &table, const gfs_sgd_params &clamped, uint64_t zlen_full, double *out) {
    const uint64_t len = std::min<uint64_t>(std::min<uint64_t>(gfs_zeta_table_len(&clamped), zlen_full), table.size());
    if (len) memcpy(out, table.data(), len * sizeof(double));
}

}  // namespace gfs
