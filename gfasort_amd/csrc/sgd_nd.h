// sgd_nd.h — the device functions of the layout's reference streams (ref_run_nd: K2, K2d, and the batch kernels of
// sgd_kernels_batch.hip).  The 1D sort's are in sgd_1d.h.
#pragma once
#include "sgd_kernel_common.h"

namespace gfs {

// Everything of one loop trip that does not depend on the coordinates: the pair sampler, the node lengths, the two end
// flips and the rejections of sgd.rs:990-1103.  Returns false where the reference `continue`s.
// Node lengths come from the step records themselves: pos[s+1]-pos[s] inside a path,
// path_len - pos[s] for a path's last step (identical to graph.nodes[id].sequence.len(),
// 0 for an absent node — sgd.rs:1051-1058 — because PathIndex positions are the exclusive
// prefix sum of exactly those lengths, sgd.rs:43-54).
struct RefTermND { uint32_t ni, nj; uint32_t ends; int crowd; double term_dist; };     // ends: bit 0 = end of i, bit 1 = end of j

template <bool LDS_TABLES>
__device__ __forceinline__ bool ref_sample_nd(const KArgs &a, const uint4 *path_tab, const double *zeta_tab, Rng &rng,
                                              const uint64_t step_idx, const uint4 &ra, RefTermND &t) {
    uint4 rb; uint64_t sa, sb; uint32_t cnt, path;
    if (!sample_pair_from<LDS_TABLES>(a, path_tab, zeta_tab, rng, step_idx, ra, rb, sa, sb, cnt, path)) return false;
    const uint64_t first = path_first(path_tab[path]);
    const uint64_t last_step = first + cnt - 1u;
    const uint64_t plen = a.path_len[path];
    uint64_t pa = rec_pos_u64(ra), pb = rec_pos_u64(rb);
    uint64_t na, nb;                       // position of the following step / path end
    if (sa == last_step) na = plen; else { uint4 n = a.step_rec[sa + 1u]; na = rec_pos_u64(n); }
    if (sb == last_step) nb = plen; else { uint4 n = a.step_rec[sb + 1u]; nb = rec_pos_u64(n); }
    double pos_a = (double)pa, pos_b = (double)pb;                                     // sgd.rs:1047-1048
    const double len_i = (double)(na - pa), len_j = (double)(nb - pb);                // :1051-1058
    const bool rev_i = (ra.y >> 31) != 0, rev_j = (rb.y >> 31) != 0;                   // :1061,1070
    bool oa = rng.flip() == 1u;                                                        // :1062
    if (oa) { pos_a += len_i; oa = !rev_i; } else { oa = rev_i; }                      // :1063-1068
    bool ob = rng.flip() == 1u;                                                        // :1071
    if (ob) { pos_b += len_j; ob = !rev_j; } else { ob = rev_j; }                      // :1072-1077
    t.term_dist = fabs(pos_a - pos_b);                                                 // :1080
    if (t.term_dist == 0.0) return false;                                              // :1081
    t.crowd = crowd_shift<false>(a, ra, rb);
    t.ni = ra.x; t.nj = rb.x;
    t.ends = (oa ? 1u : 0u) | (ob ? 2u : 0u);
    return t.ni != 0xFFFFFFFFu && t.nj != 0xFFFFFFFFu;                                 // :1089-1096
}

// The worker loop for `quota` successful updates (sgd.rs:988-1156).  As in K1 (sgd_kernels_1d.hip ref_run_1d) the next trip's
// step a is drawn, and its record requested, before the current term's adds are issued.
template <int D, bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE>
__device__ __forceinline__ void ref_run_nd(const KArgs &a, const uint4 *path_tab, const double *zeta_tab, Rng &rng,
                                           const uint32_t quota, const uint64_t max_att, const uint32_t tid,
                                           uint32_t &done, uint32_t &att, uint32_t &ntr) {
    uint32_t d = 0; uint64_t t = 0;
    uint64_t s_a = 0; uint4 r_a = make_uint4(0, 0, 0, 0); bool drawn = false;         // the next trip's step a, when drawn ahead
    while (d < quota && t < max_att) {
        ++t;
        if (!drawn) { s_a = sample_step(a, rng); r_a = a.step_rec[s_a]; }              // :990
        drawn = false;
        RefTermND cur;
        if (!ref_sample_nd<LDS_TABLES>(a, path_tab, zeta_tab, rng, s_a, r_a, cur)) continue;
        const bool oa = (cur.ends & 1u) != 0u, ob = (cur.ends & 2u) != 0u;
        const uint64_t idx_i = (uint64_t)cur.ni * 2u + (oa ? 1u : 0u);                 // :1099-1103
        const uint64_t idx_j = (uint64_t)cur.nj * 2u + (ob ? 1u : 0u);
        double *ci = coord_ptr<D>(a, cur.ni, oa), *cj = coord_ptr<D>(a, cur.nj, ob);
        const uint64_t cs = coord_step(a);
        const double mu = crowd_scale(fmin(a.it.eta * (1.0 / cur.term_dist), 1.0), cur.crowd);   // :1085-1086
        // (the step written out, not layout_step: through the helper the trace kernel at D = 8 spills a register)
        double deltas[D];
        double mag_sq = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {                                                  // :1108-1113
            deltas[k] = load_pos<ATOMIC_LOADS>(ci + k * cs) - load_pos<ATOMIC_LOADS>(cj + k * cs);
            mag_sq += deltas[k] * deltas[k];
        }
        if (mag_sq == 0.0) { deltas[0] = 1e-9; mag_sq = 1e-18; }                       // :1116-1119
        const double mag = sqrt(mag_sq);                                               // :1121
        const double delta = mu * (mag - cur.term_dist) / 2.0;                         // :1125
        const double r = delta / mag;                                                  // :1142
        const bool same = idx_i == idx_j;   // reference stores c_i-r then c_j+r from values
                                            // loaded before either store: the 2nd wins (:1145-1148)
        if (d + 1u < quota && t < max_att) { s_a = sample_step(a, rng); r_a = a.step_rec[s_a]; drawn = true; }   // the next trip's :990
#pragma unroll
        for (int k = 0; k < D; ++k) {                                                  // :1143-1149
            const double r_d = r * deltas[k];
            if (!same) add_pos(ci + k * cs, -r_d);
            add_pos(cj + k * cs, r_d);
        }
        ++d;                                                                           // :1151
        if (TRACE) record_trace(a, tid, ntr, (uint32_t)idx_i, (uint32_t)idx_j, cur.term_dist);
    }
    done += d;
    att += t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
}

}  // namespace gfs
