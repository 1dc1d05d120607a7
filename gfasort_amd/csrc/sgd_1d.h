// sgd_1d.h — the device functions of the 1D sort's samplers: reference streams (ref_run_1d: K1, K1d) and the team
// trip machine (team_iteration: K1b, K1c).  sgd_kernels_1d.hip instantiates them in K1 / K1b / K1c / K1d,
// sgd_kernels_1d_phased.hip in K1e, which switches between the two per iteration.
#pragma once
#include "sgd_kernel_common.h"

namespace gfs {

// ------------------------------------------------------------------------------------------
// K1: 1D reference streams — one lane = one reference worker thread (sgd.rs:429-590)
// ------------------------------------------------------------------------------------------
// Everything of one loop trip that does not depend on the positions: the pair sampler and the rejections of
// sgd.rs:444-538.  Returns false where the reference `continue`s.
struct RefTerm1D { uint32_t i, j; int crowd; double term_dist; };

// (step_idx, ra: the trip's step a and its record, drawn and requested by the caller — see ref_run_1d)
template <bool LDS_TABLES>
__device__ __forceinline__ bool ref_sample_1d(const KArgs &a, const uint4 *path_tab, const double *zeta_tab, Rng &rng,
                                              const uint64_t step_idx, const uint4 &ra, RefTerm1D &t) {
    uint4 rb; uint64_t sa, sb; uint32_t cnt, path;
    if (!sample_pair_from<LDS_TABLES>(a, path_tab, zeta_tab, rng, step_idx, ra, rb, sa, sb, cnt, path)) return false;
    t.term_dist = fabs(rec_pos(ra) - rec_pos(rb));                                     // sgd.rs:513
    if (t.term_dist == 0.0) return false;                                              // :514
    t.crowd = crowd_shift<false>(a, ra, rb);
    t.i = ra.x; t.j = rb.x;
    return t.i != 0xFFFFFFFFu && t.j != 0xFFFFFFFFu;                                   // :525-538
}

// The worker loop for `quota` successful updates (sgd.rs:442-584).
// ONE thing is moved: the draw of the NEXT trip's step a (sgd.rs:444 — the next random number in the stream's order whatever
// happens in between) and the request of its record are issued BEFORE the current term's two adds instead of after them.
// vmcnt counts in order on gfx9: a load issued after the adds cannot be seen to complete before the adds have completed at the
// memory side (~1.5 us), and that wait was on every update's critical path; a load issued before them can.  Records are
// read-only, positions are still read after the previous term's adds: one stream is bit for bit the oracle's (tested), and a
// term is in flight no longer than before.  (Round 3 first overlapped the WHOLE next sample with the position loads: no faster,
// and a term's positions were then read ~1 us earlier — more terms in flight per stream, which the streams-per-node bound
// exists to limit: a tandem-repeat graph stable at the bound diverged.  profiles/r03/ref_fused_probe.log, repeat_stability.log.)
template <bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE>
__device__ __forceinline__ void ref_run_1d(const KArgs &a, const uint4 *path_tab, const double *zeta_tab, Rng &rng,
                                           const uint32_t quota, const uint64_t max_att, const uint32_t tid,
                                           uint32_t &done, uint32_t &att, uint32_t &ntr) {
    double *x = a.x;
    uint32_t d = 0; uint64_t t = 0;
    uint64_t s_a = 0; uint4 r_a = make_uint4(0, 0, 0, 0); bool drawn = false;         // the next trip's step a, when drawn ahead
    while (d < quota && t < max_att) {
        ++t;
        if (!drawn) { s_a = sample_step(a, rng); r_a = a.step_rec[s_a]; }              // :444
        drawn = false;
        RefTerm1D cur;
        if (!ref_sample_1d<LDS_TABLES>(a, path_tab, zeta_tab, rng, s_a, r_a, cur)) continue;
        const double mu = crowd_scale(fmin(a.it.eta * (1.0 / cur.term_dist), 1.0), cur.crowd);   // :518-520
        double dx;
        if (a.dbg & 2u) dx = (double)cur.i - (double)cur.j;                            // ablation: no position loads
        else dx = load_pos<ATOMIC_LOADS>(x + cur.i) - load_pos<ATOMIC_LOADS>(x + cur.j);   // :541-543
        if (dx == 0.0) dx = 1e-9;                                                      // :546-548
        const double mag = fabs(dx);                                                   // :551
        const double delta = mu * (mag - cur.term_dist) / 2.0;                         // :552
        const double r = delta / mag;                                                  // :570
        const double r_x = r * dx;                                                     // :571
        if (d + 1u < quota && t < max_att) { s_a = sample_step(a, rng); r_a = a.step_rec[s_a]; drawn = true; }   // the next trip's :444
        if (a.dbg & 1u) { asm volatile("" :: "v"(r_x)); }                              // ablation: no atomics
        else {
            add_pos(x + cur.i, -r_x);                                                  // :575
            add_pos(x + cur.j, r_x);                                                   // :576
        }
        ++d;                                                                           // :579
        if (TRACE) record_trace(a, tid, ntr, cur.i, cur.j, cur.term_dist);
    }
    done += d;
    att += t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
}

// ------------------------------------------------------------------------------------------
// K1b: 1D team kernel — bundled ("run") sampling (sgd_device.h).  A wave is a team:
//   pass   : all 64 lanes sample one leader term each from their own reference streams — the
//            Zipf/f64 arithmetic runs at full SIMD width instead of on one lane per bundle;
//   trips  : the leaders are executed one slot after the other, each as 64/B runs of B lanes.  With B = 64 a
//            leader's run extends over K consecutive trips (LONG RUNS, sgd_device.h run_trips); a leader whose
//            jump is shorter than a trip runs for one trip only and both of its colours (two_colour) are computed in
//            that trip (fused_trip), or in two trips where it touches a path end.  The records of the next
//            trip are requested before the current one is consumed, so a trip exposes one memory round trip
//            (its position loads); its adds are issued at once and never waited for by themselves.
//            (Round 1 issued a trip's adds one trip late, behind the next trip's loads; with long runs — whose
//            next trip touches the neighbouring lines — that was slower, 66.8 vs 73.4 G updates/s on C3, and it
//            let a wave read positions it was about to change: profiles/r02/quality_probe_defer.log.)
// The quota is per WAVE with a rank cut-off in the last trip: an iteration performs exactly its
// number of updates; what is left of a pass when the quota fills serves the next iteration (TeamState).
// ------------------------------------------------------------------------------------------
// Per-wave state that survives from one iteration to the next inside a launch.
struct TeamState {
    Rng rng;
    // the wave's current pass: 64 leaders (one per lane) of which `left` trip slots have not been fully expanded yet
    // (`colour` = 1: the current slot's first colour is done, its second is next — sgd_device.h two_colour).
    // A pass outlives the iteration it was sampled in (eta is not part of sampling); it is dropped when
    // the cooling phase — the only thing the sampler depends on besides the RNG — changes.
    Leader L = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t left = 0, cool = 0, colour = 0, seg = 0;   // seg: next trip of the current slot's run (sgd_device.h run_trips)
    uint32_t p = 0;                                     // partner of the current slot's leader the next trip belongs to
    uint32_t done = 0, att = 0, ntr = 0;
};

// The record of a step as a trip reads it: the slot, the bp position, the crowding exponents — of the 16-byte step record, or
// (COMPACT) of the 8-byte trip record { slot, pos lo } that the index build writes beside it.  The host picks COMPACT only where
// every step's high position word and every term's crowding shift are zero (launch_policy.h compact_records): then the two
// widths give the same values bit for bit, from half the record bytes and half the registers (a Trip holds three records).
// The sampler (sample_leader, draw_partner) needs the path of its step and stays on step records.
template <bool COMPACT> struct TripRec;
template <> struct TripRec<false> {
    uint4 r = make_uint4(0, 0, 0, 0);
    static __device__ __forceinline__ TripRec load(const KArgs &a, uint64_t s) { TripRec t; t.r = a.step_rec[s]; return t; }
    __device__ __forceinline__ uint32_t slot() const { return r.x; }
    __device__ __forceinline__ double pos() const { return rec_pos(r); }
    static __device__ __forceinline__ int crowd(const KArgs &a, const TripRec &ra, const TripRec &rb) { return crowd_shift<true>(a, ra.r, rb.r); }
};
template <> struct TripRec<true> {
    uint2 r = make_uint2(0, 0);
    static __device__ __forceinline__ TripRec load(const KArgs &a, uint64_t s) { TripRec t; t.r = a.trip_rec[s]; return t; }
    __device__ __forceinline__ uint32_t slot() const { return r.x; }
    __device__ __forceinline__ double pos() const { return (double)r.y; }
    static __device__ __forceinline__ int crowd(const KArgs &, const TripRec &, const TripRec &) { return 0; }
};

// One trip = (slot t of the pass, trip seg of its run, partner, colour): what every lane needs to execute it.
template <bool COMPACT>
struct Trip {
    uint64_t sa = 0, sb = 0;
    TripRec<COMPACT> ra, rb;
    TripRec<COMPACT> rc;       // twin trip: the record of the second partner's step
    bool twin = false;         // wave-uniform: both partners of an aligned leader in ONE trip (twin_trip)
    bool valid = false;        // this lane acts in the trip (fused trip: this lane's partner lies beyond the trip's 64 steps)
    int mshift = 0;            // != 0: merged short-jump trip (sgd_kernel_common.h merged_trip_shift)
    bool two = false;          // wave-uniform: some run of this slot has a second colour
    bool fused = false;        // wave-uniform: both colours of a short-jump run in ONE trip (fused_trip)
    uint32_t k = 1;            // wave-uniform: trips of this slot's run (long runs: B = 64 only)
    uint32_t off = 0;          // wave-uniform: this trip starts `off` steps after the run's first step (run_offset)
};

template <int B, bool COMPACT>
__device__ __forceinline__ void expand_trip(const KArgs &a, const Leader &L, int t, uint32_t seg, uint32_t p, uint32_t colour, int sub, int q, Trip<COMPACT> &tr) {
    using Rec = TripRec<COMPACT>;
    constexpr int RUNS = 64 / B;
    const int ll = t * RUNS + q;
    const uint32_t okw = bcast<B>(L.ok, ll), cnt = bcast<B>(L.cnt, ll);
    const uint32_t ok = leader_ok(okw, p);
    const uint32_t ra0 = p ? bcast<B>(L.ra1, ll) : bcast<B>(L.ra0, ll), rb0 = p ? bcast<B>(L.rb1, ll) : bcast<B>(L.rb0, ll);
    const uint64_t first = bcast_first<B>(L, ll);
    // long runs only where the whole wave follows one leader; a leader the reference rejected takes one (empty) trip.
    // (The number of trips must not depend on the partner: the trips of a slot go seg by seg, both partners each.)
    tr.k = (B == 64 && ((okw | (okw >> 8)) & 1u) && cnt >= 2u * B) ? run_trips(a.chain, (uint32_t)B, cnt) : 1u;
    tr.off = B == 64 ? run_offset((uint32_t)B, cnt, tr.k, ra0, rb0, seg) : 0u;
    tr.mshift = merged_trip_shift<B>(ok, cnt, ra0, rb0, tr.off);
    const bool two = !(a.dbg & 0x08u) && two_colour<B>(ok, cnt, ra0, rb0);
    tr.two = B == 64 ? two : (__any(two) != 0);                       // B = 64: the leader is wave-uniform already
    tr.ra = Rec(); tr.rb = Rec(); tr.rc = Rec();
    tr.fused = B == 64 && tr.mshift != 0 && colour == 0 && two && !(a.dbg & 0x100u);
    // both partners line-aligned long jumps: their a-runs are the same blocks (draw_partner), one trip serves both
    tr.twin = B == 64 && p == 0u && a.partners == 2u && (okw & 3u) == 3u && ((okw >> 8) & 3u) == 3u && !(a.dbg & 0x04u);
    const uint32_t rb1 = bcast<B>(L.rb1, ll);
    if (tr.twin) {
        // ... unless a block of one partner run lies within two trips of the other's (|gap| < 192 steps): the wave would read, as
        // one partner's positions, what it has only just added as the other's — in the same trip from the very snapshot the
        // add was computed from (no-return atomics are posted).  Partner runs further apart may overlap as runs: their common
        // nodes are then read two or more trips after they were added to.  (With round 1's free-running launch such leaders as
        // twin trips cost the 525k-node bubble graph a quarter of its precision at path distance 1, profiles/r02/two_partners.log.)
        const int64_t gap = (int64_t)rb0 - (int64_t)rb1, lim = 192;
        if (gap < lim && gap > -lim) tr.twin = false;
    }
    if (tr.twin) {
        tr.sa = first + ra0 + tr.off + (uint32_t)sub;
        tr.sb = first + rb0 + tr.off + (((uint32_t)sub + ((okw >> 2) & 7u)) & 63u);
        const uint64_t sc = first + rb1 + tr.off + (((uint32_t)sub + ((okw >> 10) & 7u)) & 63u);
        tr.valid = true;
        tr.ra = Rec::load(a, tr.sa); tr.rb = Rec::load(a, tr.sb); tr.rc = Rec::load(a, sc);
        return;
    }
    if (tr.fused) {
        // every lane takes its own step of the trip and its partner's record (the partners inside the trip are the other
        // lanes' own steps: the same lines, no extra traffic; merged_trip_shift guarantees all of them lie in the path)
        const int dst = sub + tr.mshift;
        tr.sa = first + merged_trip_base(cnt, ra0, tr.off) + (uint32_t)sub;
        tr.sb = (uint64_t)((int64_t)tr.sa + tr.mshift);
        tr.valid = dst < 0 || dst > 63;
        tr.ra = Rec::load(a, tr.sa);
        tr.rb = Rec::load(a, tr.sb);
        return;
    }
    tr.valid = expand_run<B>(ok, first, cnt, ra0, rb0, sub, colour, tr.off, tr.sa, tr.sb);
    if (tr.valid) { tr.ra = Rec::load(a, tr.sa); tr.rb = Rec::load(a, tr.sb); }
}

// The term arithmetic of sgd.rs:518-571 on values already in registers; returns r_x.
__device__ __forceinline__ double term_move(const KArgs &a, double term_dist, double xi, double xj, int crowd) {
    double mu = crowd_scale(fmin(a.it.eta * (1.0 / term_dist), 1.0), crowd);          // :518-520
    double dx = xi - xj;                                                               // :543
    if (dx == 0.0) dx = 1e-9;                                                          // :546-548
    double mag = fabs(dx);                                                             // :551
    double delta = mu * (mag - term_dist) / 2.0;                                       // :552
    double r = delta / mag;                                                            // :570
    return r * dx;                                                                     // :571
}

__device__ __forceinline__ double shfl_f64(double v, int src) { return __shfl(v, src, 64); }

// FUSED short-jump trip (B = 64, |jump| = z < 64, the run's 64 steps and all their partners inside the path).
// The run's 64 terms (l, l+s) form two node-disjoint colours (two_colour).  As two trips, each colour loads the records
// and positions of half the lanes and of their partners — which are the OTHER colour's lanes — and the second colour
// reads what the first one wrote.  Here every lane loads its own record and position once; partners inside the run are
// read from the lane that holds them (wave shuffles), colour 1 computes on the positions colour 0 has just produced in
// registers (bit for bit what it would read back from memory when no other wave interferes), and a lane's node takes ONE
// add for both colours — what it gave as the acting lane of one colour plus what it took as the partner in the other:
// memory receives x + (-r + r') where two trips would make it (x - r) + r' (the oracle's mirror rounds the same way).
// Same terms, same arithmetic, same order as the two trips.  It buys precision under concurrency — both colours see ONE
// snapshot of the run's 64 nodes and land in one memory round trip, instead of exposing the run to the other ~5 000 waves
// for two: at one stream per two nodes (525k-node bubble graph) the relative error at path distance 1 is 0.200 against
// 0.248 with two trips (reference streams: 0.194; profiles/r02/quality_probe_long_runs.log) — and, since the one add per node, speed: the kernel is bound by the memory side's atomic units,
// and a fused trip now costs 8 requests for 64 updates where two trips cost 16 (C3 80.0 -> 87.4 G updates/s, bubble
// graphs 49.9 -> 53.6 and 52.0 -> 55.8: profiles/r02/fused_trip_one_add.log).  Returns false when the wave's quota filled
// before the second colour: the caller leaves that colour to the next iteration as a generic trip.
template <bool ATOMIC_LOADS, bool TRACE, bool COMPACT>
__device__ __forceinline__ bool fused_trip(const KArgs &a, TeamState &ts, const Trip<COMPACT> &cur, const int lane,
                                           const uint32_t tid, const uint64_t wave_quota, uint64_t &wave_done) {
    double *x = a.x;
    const int s = cur.mshift, z = s < 0 ? -s : s;
    const int dst = lane + s, src = lane - s;                          // my partner's lane; the lane whose partner I am
    const bool out = cur.valid;                                        // partner beyond the trip's 64 steps
    const int dstc = out ? lane : dst, srcc = (src < 0 || src > 63) ? lane : src;
    const uint32_t grp = ((cur.off + (uint32_t)lane) / (uint32_t)z) & 1u;
    const uint32_t node = cur.ra.slot(), pnode = cur.rb.slot();
    double xo = 0.0, xp = 0.0;                                         // my position; my partner's when it is beyond the trip
    if (!(a.dbg & 2u)) {
        if (node != 0xFFFFFFFFu) xo = load_pos<ATOMIC_LOADS>(x + node);
        if (out && pnode != 0xFFFFFFFFu) xp = load_pos<ATOMIC_LOADS>(x + pnode);       // (partners inside: from their lanes)
    } else { xo = (double)node; xp = (double)pnode; }
    const double term_dist = fabs(cur.ra.pos() - cur.rb.pos());                        // sgd.rs:513
    const int crowd = TripRec<COMPACT>::crowd(a, cur.ra, cur.rb);
    const bool term_ok = term_dist != 0.0 && node != 0xFFFFFFFFu && pnode != 0xFFFFFFFFu;   // :514, :525-538
    double acc = 0.0;
    bool touched = false, second = true;
#pragma unroll
    for (uint32_t colour = 0; colour < 2u; ++colour) {
        ++ts.att;
        const bool valid = quota_cut(term_ok && grp == colour, lane, wave_quota, wave_done);
        const double xpart_in = shfl_f64(xo, dstc);                    // partner's CURRENT position (colour 0's result for colour 1)
        const double xj = out ? xp : xpart_in;
        double r_x = 0.0;
        if (valid) {
            r_x = term_move(a, term_dist, xo, xj, crowd);
            ++ts.done;                                                                 // :579
            if (TRACE) record_trace(a, tid, ts.ntr, node, pnode, term_dist);
        }
        // the +r of the lane whose partner I am
        // (every shuffle is a statement of its own: inside `a && __shfl(..)` or `c ? x : __shfl(..)` the compiler may run it
        // only on the lanes that need the result, and a SOURCE lane that is switched off then supplies nothing)
        const double rv = shfl_f64(r_x, srcc);
        const int vsrc = __shfl((int)valid, srcc, 64);
        const bool recv = src >= 0 && src <= 63 && vsrc != 0;
        // a lane acts or receives in a colour, never both (its group's parity decides)
        if (valid) xo = xo - r_x;                                                      // :575  x[i] - r_x
        if (recv) xo = xo + rv;                                                        // :576  x[j] + r_x
        // a lane's own node takes ONE add for both colours, the sum of what it gave as an acting lane in one colour and
        // took as a partner in the other (its register holds (x - r) + r', memory receives x + (-r + r')): half the
        // atomic requests of the trip
        if (valid) { acc = touched ? acc - r_x : -r_x; touched = true; }
        if (recv) { acc = touched ? acc + rv : rv; touched = true; }
        if (valid && out && !(a.dbg & 1u)) add_pos(x + pnode, r_x);                    // partner beyond the trip
        if (colour == 0 && wave_done >= wave_quota) { second = false; break; }
    }
    if (touched && !(a.dbg & 1u)) add_pos(x + node, acc);
    return second;
}

// TWIN trip (B = 64, two partners, both line-aligned long jumps: sgd_device.h Leader).  A lane's step a is the a-side of two
// terms, (a, b) and (a, c), b and c in two other aligned blocks of the path.  One load of a's record and position serves
// both; the second term computes on what the first left in the register, as it would read it back from memory; a's node
// takes ONE add, -(r + r'), b and c one each: 3 blocks of 8 requests for 128 updates where two trips take 4.  Returns false
// when the wave's quota filled before the second term: the caller leaves the second partner's trip to the next iteration.
template <bool ATOMIC_LOADS, bool TRACE, bool COMPACT>
__device__ __forceinline__ bool twin_trip(const KArgs &a, TeamState &ts, const Trip<COMPACT> &cur, const int lane,
                                          const uint32_t tid, const uint64_t wave_quota, uint64_t &wave_done) {
    double *x = a.x;
    const uint32_t node = cur.ra.slot(), nb = cur.rb.slot(), nc = cur.rc.slot();
    double xa = 0.0, xb = 0.0, xc = 0.0;
    if (!(a.dbg & 2u)) {
        if (node != 0xFFFFFFFFu) xa = load_pos<ATOMIC_LOADS>(x + node);
        if (nb != 0xFFFFFFFFu) xb = load_pos<ATOMIC_LOADS>(x + nb);
        if (nc != 0xFFFFFFFFu) xc = load_pos<ATOMIC_LOADS>(x + nc);
    } else { xa = (double)node; xb = (double)nb; xc = (double)nc; }
    const double pa = cur.ra.pos();
    double acc = 0.0;
    bool touched = false, second = true;
#pragma unroll
    for (uint32_t p = 0; p < 2u; ++p) {
        ++ts.att;
        const TripRec<COMPACT> &rp = p ? cur.rc : cur.rb;
        const uint32_t pn = p ? nc : nb;
        const double term_dist = fabs(pa - rp.pos());                                  // sgd.rs:513
        const bool valid = quota_cut(term_dist != 0.0 && node != 0xFFFFFFFFu && pn != 0xFFFFFFFFu,   // :514, :525-538
                                     lane, wave_quota, wave_done);
        if (valid) {
            const double r_x = term_move(a, term_dist, xa, p ? xc : xb, TripRec<COMPACT>::crowd(a, cur.ra, rp));   // :518-571
            ++ts.done;                                                                 // :579
            if (TRACE) record_trace(a, tid, ts.ntr, node, pn, term_dist);
            xa = xa - r_x;                                                             // :575
            acc = touched ? acc - r_x : -r_x; touched = true;
            if (!(a.dbg & 1u)) add_pos(x + pn, r_x);                                   // :576
        }
        if (p == 0u && wave_done >= wave_quota) { second = false; break; }
    }
    if (touched && !(a.dbg & 1u)) add_pos(x + node, acc);
    return second;
}

// One SGD iteration of one wave: passes and trips until the wave's quota is filled.
// (COMPACT: the trips read 8-byte trip records, TripRec; B = 64 only)
template <int B, bool LDS_TABLES, bool ATOMIC_LOADS, bool TRACE, bool COMPACT = false>
__device__ __forceinline__ void team_iteration(const KArgs &a, const uint4 *path_tab, const double *zeta_tab,
                                               TeamState &ts, const uint32_t tid, const uint64_t wave_quota, const IterConsts *itp = nullptr) {
    static_assert(B == 64 || !COMPACT, "trip records are read by the trips of B = 64 only");
    const int lane = threadIdx.x & 63;
    const int sub = lane & (B - 1);
    const int q = lane / B;
    const uint64_t max_passes = (uint64_t)a.attempt_factor * (wave_quota / (64u * B) + 1u) + 16u;
    uint64_t wave_done = 0, passes = 0;
    double *x = a.x;
    while (wave_done < wave_quota && passes < max_passes) {
        if (ts.left == 0 || ts.cool != (uint32_t)a.it.cooling) {
            ++passes;
            // (the sampler reads its launch constants afresh — sgd_kernel_common.h reload_kargs — and, in a fused launch, the
            // iteration's constants from the schedule in memory: itp)
            KArgs as;
            reload_kargs(as);
            if (itp) {
                const IterConsts *ip = itp;
                asm volatile("" : "+s"(ip));
                as.it = *ip;
            }
            ts.L = sample_leader<LDS_TABLES>(as, path_tab, zeta_tab, ts.rng);
            ts.left = B; ts.cool = (uint32_t)a.it.cooling; ts.colour = 0; ts.seg = 0; ts.p = 0;
        }
        const Leader &L = ts.L;
        int t = B - (int)ts.left;
        uint32_t colour = ts.colour, seg = ts.seg, p = ts.p;
        Trip<COMPACT> cur;
        expand_trip<B>(a, L, t, seg, p, colour, sub, q, cur);          // expand and request the records of the first trip
        for (;;) {
            // the trip after this one: this trip's second colour (unless fused into it), else the same trip of the run for
            // the leader's second partner (unless this is a twin trip), else the run's next trip, else the next slot;
            // request its records now
            int t_n = t; uint32_t colour_n = 0u, seg_n = seg, p_n = p;
            if (colour == 0 && cur.two && !cur.fused) colour_n = 1u;
            else if (p == 0u && a.partners == 2u && !cur.twin) p_n = 1u;
            else if (seg + 1u < cur.k) { seg_n = seg + 1u; p_n = 0u; }
            else { t_n = t + 1; seg_n = 0u; p_n = 0u; }
            const bool have_n = t_n < B;
            Trip<COMPACT> nxt;
            if (have_n) expand_trip<B>(a, L, t_n, seg_n, p_n, colour_n, sub, q, nxt);
            if (B == 64 && cur.twin) {
                if (!twin_trip<ATOMIC_LOADS, TRACE>(a, ts, cur, lane, tid, wave_quota, wave_done)) {
                    ts.colour = 0u; ts.seg = seg; ts.p = 1u;           // quota filled between the partners: the second one
                    break;                                             // is the next iteration's first trip (generic form)
                }
                ts.colour = 0u; ts.seg = seg_n; ts.p = 0u;
                if (t_n != t) --ts.left;
                if (wave_done >= wave_quota || !have_n) break;
                cur = nxt; t = t_n; colour = colour_n; seg = seg_n; p = p_n;
                continue;
            }
            if (B == 64 && cur.fused) {
                if (!fused_trip<ATOMIC_LOADS, TRACE>(a, ts, cur, lane, tid, wave_quota, wave_done)) {
                    ts.colour = 1u; ts.seg = seg; ts.p = p;            // quota filled between the colours: the second one is
                    break;                                             // the next iteration's first trip (generic form)
                }
                ts.colour = 0u; ts.seg = seg_n; ts.p = p_n;
                if (t_n != t) --ts.left;
                if (wave_done >= wave_quota || !have_n) break;
                cur = nxt; t = t_n; colour = colour_n; seg = seg_n; p = p_n;
                continue;
            }
            // consume the current trip
            ++ts.att;
            ts.colour = colour_n; ts.seg = seg_n; ts.p = p_n;
            if (t_n != t) --ts.left;
            bool valid = cur.valid;
            const TripRec<COMPACT> ra = cur.ra, rb = cur.rb;
            const int mshift = cur.mshift;
            double term_dist = 0.0;
            uint32_t i = 0, j = 0;
            if (valid) {
                term_dist = fabs(ra.pos() - rb.pos());                                 // sgd.rs:513
                i = ra.slot(); j = rb.slot();
                valid = term_dist != 0.0 && i != 0xFFFFFFFFu && j != 0xFFFFFFFFu;      // :514, :525-538
            }
            valid = quota_cut(valid, lane, wave_quota, wave_done);
            double xi = 0.0, xj = 0.0;
            if (valid) {
                if (a.dbg & 2u) { xi = (double)i; xj = (double)j; }                    // ablation: no position loads
                else { xi = load_pos<ATOMIC_LOADS>(x + i); xj = load_pos<ATOMIC_LOADS>(x + j); }   // :541-542
            }
            double r_x = 0.0;
            if (valid) {
                r_x = term_move(a, term_dist, xi, xj, TripRec<COMPACT>::crowd(a, ra, rb));   // :518-571
                ++ts.done;                                                             // :579
                if (TRACE) record_trace(a, tid, ts.ntr, i, j, term_dist);
            }
            // the adds of this trip (:575-576): -r_x to node i, +r_x to node j
            bool o1f = valid, o2f = valid; uint32_t o1s = i, o2s = j; double o1v = -r_x, o2v = r_x;
            if (B == 64 && mshift != 0) {
                // merged short-jump trip (wave-uniform branch): a resting lane takes over the +r of the acting lane
                // whose partner is the step it sits on
                const int z = mshift < 0 ? -mshift : mshift;
                const int src = lane - mshift;                                         // the lane whose partner I sit on
                const int srcc = src < 0 ? 0 : (src > 63 ? 63 : src);
                const double rv = __shfl(r_x, srcc, 64);
                const uint32_t js = (uint32_t)__shfl((int)j, srcc, 64);
                const int vs = __shfl((int)valid, srcc, 64);
                const bool resting = (((cur.off + (uint32_t)lane) / (uint32_t)z) & 1u) != colour;
                if (resting && src >= 0 && src < 64 && vs) { o1f = true; o1s = js; o1v = rv; }
                const int dst = lane + mshift;                                         // where my own partner sits
                o2f = valid && (dst < 0 || dst > 63);                                  // beyond the run: add it myself
            }
            if (!(a.dbg & 1u)) {                                                       // (ablation: no atomics)
                if (o1f) add_pos(x + o1s, o1v);
                if (o2f) add_pos(x + o2s, o2v);
            }
            if (wave_done >= wave_quota) break;                                        // what is left of the pass serves the next iteration
            if (!have_n) break;
            cur = nxt; t = t_n; colour = colour_n; seg = seg_n; p = p_n;
        }
    }
}

}  // namespace gfs
