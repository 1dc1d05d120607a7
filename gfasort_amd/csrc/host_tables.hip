// host_tables.hip — the part of the C ABI (include/gfasort_hip.h) that is host arithmetic and nothing else: the tables, starts and
// orders that must equal the reference's bit for bit, the sample stream of the stress read-out, the batch planner, and the error
// slot.  No HIP call and no HIP header: the library builds it with the flags of the other units (-ffp-contract=off is what keeps
// the tables exact), and a plain C++17 compiler builds it as well (tests/test_launch_policy_host.py, under sanitizers).
#include "../../include/gfasort_hip.h"
#include "batch_plan.h"
#include "capi_error.h"
#include "sgd_limits.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>

using gfs::h_sat_i32;
using gfs::splitmix64;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
int gfs_set_error(int code, const std::string &msg) { return fail(code, msg); }      // for capi.hip and multi.hip

// ---- host restatements (bit-exact; this TU is built with -ffp-contract=off) ----------------
static double h_fpp(double a, double b) {                                  // sgd.rs:155-182
    int32_t e = h_sat_i32(b);
    uint64_t bits; std::memcpy(&bits, &a, 8);
    int32_t high = (int32_t)(bits >> 32);
    int32_t diff = (int32_t)((uint32_t)high - 1072632447u);
    int32_t new_high = h_sat_i32((b - (double)e) * (double)diff + 1072632447.0);
    uint64_t fb = ((uint64_t)(uint32_t)new_high) << 32;
    double frac; std::memcpy(&frac, &fb, 8);
    double base = a, r = 1.0;
    int32_t ex = e;
    if (ex < 0) return std::nan("");     // the reference would loop forever (b < 0 never occurs for theta in [0,1))
    while (ex != 0) { if (ex & 1) r *= base; base *= base; ex >>= 1; }
    return r * frac;
}

extern "C" {

const char *gfs_last_error(void) { return g_err.c_str(); }

double gfs_fast_precise_pow(double a, double b) { return h_fpp(a, b); }

int gfs_sgd_schedule(const gfs_sgd_params *p, double *etas) {              // sgd.rs:300-308,617-638
    if (!p || !etas) return fail(GFS_E_ARG, "null argument");
    double w_min = 1.0 / p->eta_max, w_max = 1.0;
    double eta_max = 1.0 / w_min;
    double eta_min = p->eps / w_max;
    double lambda = std::log(eta_max / eta_min) / ((double)p->iter_max - 1.0);
    for (uint64_t t = 0; t <= p->iter_max; ++t) {
        int64_t d = (int64_t)t - (int64_t)p->iter_with_max_learning_rate;
        if (d < 0) d = -d;
        etas[t] = eta_max * std::exp(-lambda * (double)d);
    }
    return GFS_OK;
}

// The default window of GFS_F_PHASED: around the reference's switch to the cooling phase (sgd.rs:297: cooling for
// k > first_cooling = floor(cooling_start * iter_max)), scaled with iter_max.  [first_cooling + 1 + lo, first_cooling + 1 + hi)
// with lo, hi in thousandths of iter_max (hi = kPhaseWindowToEnd: to the end of the schedule), clipped to [0, iter_max + 1).
// Chosen on DRB1-3123 x120 and a 525k-node bubble graph (profiles/r05/phased_window_probe.log).
static constexpr int64_t kPhaseWindowLo = 0, kPhaseWindowToEnd = INT64_MAX, kPhaseWindowHi = kPhaseWindowToEnd;
int gfs_phase_window(const gfs_sgd_params *p, uint64_t *k_begin, uint64_t *k_end) {
    if (!p || !k_begin || !k_end) return fail(GFS_E_ARG, "null argument");
    const unsigned __int128 n = p->iter_max, last = n + 1;                 // iterations 0..=iter_max
    const double fc = std::floor(p->cooling_start * (double)p->iter_max);   // as launch_policy.h iter_consts
    const unsigned __int128 f1 = (!(fc > 0.0) ? 0 : (fc >= 18446744073709551616.0 ? (unsigned __int128)UINT64_MAX : (unsigned __int128)(uint64_t)fc)) + 1;
    auto at = [&](int64_t per_mille) -> unsigned __int128 {                // f1 + per_mille * iter_max / 1000, clipped to [0, last]
        if (per_mille == kPhaseWindowToEnd) return last;
        const unsigned __int128 off = n * (unsigned __int128)(per_mille < 0 ? -per_mille : per_mille) / 1000;
        const unsigned __int128 v = per_mille < 0 ? (off >= f1 ? 0 : f1 - off) : f1 + off;
        return v < last ? v : last;
    };
    const unsigned __int128 e = at(kPhaseWindowHi), b = std::min(at(kPhaseWindowLo), e);
    const unsigned __int128 cap = (unsigned __int128)UINT64_MAX;           // (iter_max = 2^64 - 1: iter_max + 1 does not fit)
    *k_begin = (uint64_t)std::min(b, cap); *k_end = (uint64_t)std::min(e, cap);
    return GFS_OK;
}

uint64_t gfs_zeta_table_len(const gfs_sgd_params *p) {                     // sgd.rs:311-315
    if (!p || p->space_quantization_step == 0) return 0;
    uint64_t n = p->space <= p->space_max
                     ? p->space
                     : p->space_max + (p->space - p->space_max) / p->space_quantization_step + 1;
    return n + 1;
}

int gfs_zeta_table(const gfs_sgd_params *p, double *zetas) {               // sgd.rs:317-331
    if (!p || !zetas) return fail(GFS_E_ARG, "null argument");
    uint64_t len = gfs_zeta_table_len(p);
    if (!len) return fail(GFS_E_ARG, "bad zeta parameters");
    for (uint64_t k = 0; k < len; ++k) zetas[k] = 0.0;
    double zeta_tmp = 0.0;
    for (uint64_t i = 1; i <= p->space; ++i) {
        zeta_tmp += h_fpp(1.0 / (double)i, p->theta);
        if (i <= p->space_max) zetas[i] = zeta_tmp;
        if (i >= p->space_max && (i - p->space_max) % p->space_quantization_step == 0) {
            uint64_t idx = p->space_max + 1 + (i - p->space_max) / p->space_quantization_step;
            if (idx < len) zetas[idx] = zeta_tmp;
        }
    }
    return GFS_OK;
}

int gfs_init_positions(const gfs_graph_view *g, double *x) {               // sgd.rs:271-294
    if (!g || (!x && g->n_nodes)) return fail(GFS_E_ARG, "null argument");
    uint64_t len = 0;
    for (uint64_t i = 0; i < g->n_nodes; ++i) { x[i] = (double)len; len += g->node_len[i]; }
    return GFS_OK;
}

int gfs_init_layout_dim0(const gfs_graph_view *g, uint64_t D, double *c) { // sgd.rs:832-853
    if (!g || (!c && g->n_nodes) || D == 0) return fail(GFS_E_ARG, "bad argument");
    uint64_t len = 0;
    for (uint64_t i = 0; i < g->n_nodes; ++i) {
        c[i * 2 * D + 0] = (double)len;
        c[i * 2 * D + D] = (double)(len + g->node_len[i]);
        len += g->node_len[i];
    }
    return GFS_OK;
}

// rand_distr 0.5 StandardNormal (f64) on Xoshiro256+ — the 256-layer ziggurat, restated from the crate's published
// algorithm; its tables are rebuilt by the construction of the crate's generator script (R, V below).  PARITY UNPINNED
// (DESIGN.md §5): neither the crate nor its table literals are in the container.
namespace {
constexpr double kZigR = 3.6541528853610088, kZigV = 0.00492867323399;
struct ZigTables {
    double x[257], f[257];
    ZigTables() {
        x[0] = kZigV / std::exp(-kZigR * kZigR / 2.0);
        x[1] = kZigR;
        for (int i = 1; i < 256; ++i) x[i + 1] = std::sqrt(-2.0 * std::log(kZigV / x[i] + std::exp(-x[i] * x[i] / 2.0)));
        x[256] = 0.0;
        for (int i = 0; i <= 256; ++i) f[i] = std::exp(-x[i] * x[i] / 2.0);
    }
};
struct Xo256p {                                                            // rand_xoshiro 0.7 Xoshiro256Plus
    uint64_t s[4];
    explicit Xo256p(uint64_t seed) { for (auto &w : s) w = splitmix64(seed); }   // seed_from_u64
    uint64_t next() {
        const uint64_t r = s[0] + s[3], t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = (s[3] << 45) | (s[3] >> 19);
        return r;
    }
    uint64_t uniform_usize(uint64_t n) {                                       // rand 0.9 Uniform<usize>::new(0, n): the u32 sampler
        if (n <= 0xFFFFFFFFull) {                                              // where n fits, widening multiply and rejection
            const uint32_t range = (uint32_t)n, thresh = (uint32_t)(0u - range) % range;
            for (;;) { const uint64_t m = (uint64_t)(uint32_t)(next() >> 32) * range; if ((uint32_t)m >= thresh) return m >> 32; }
        }
        const uint64_t thresh = (0ull - n) % n;
        for (;;) { const unsigned __int128 m = (unsigned __int128)next() * n; if ((uint64_t)m >= thresh) return (uint64_t)(m >> 64); }
    }
};
inline double float_with_exponent(uint64_t fraction52, int e) {
    const uint64_t b = fraction52 | ((uint64_t)(1023 + e) << 52);
    double d; std::memcpy(&d, &b, 8); return d;
}
inline double open01(Xo256p &g) { return float_with_exponent(g.next() >> 12, 0) - (1.0 - 2.220446049250313e-16 / 2.0); }
double standard_normal(Xo256p &g) {
    static const ZigTables T;
    for (;;) {
        const uint64_t bits = g.next();
        const unsigned i = (unsigned)(bits & 0xff);
        const double u = float_with_exponent(bits >> 12, 1) - 3.0;               // [-1, 1)
        const double x = u * T.x[i];
        if (std::fabs(x) < T.x[i + 1]) return x;
        if (i == 0) {                                                          // the tail beyond R
            double tx = 1.0, ty = 0.0;
            while (-2.0 * ty < tx * tx) {
                const double x_ = open01(g), y_ = open01(g);
                tx = std::log(x_) / kZigR; ty = std::log(y_);
            }
            return u < 0.0 ? tx - kZigR : kZigR - tx;
        }
        const double r = (double)(g.next() >> 11) * (1.0 / 9007199254740992.0);  // rng.random::<f64>()
        if (T.f[i + 1] + (T.f[i] - T.f[i + 1]) * r < std::exp(-x * x / 2.0)) return x;
    }
}
}  // namespace

// The whole start of path_linear_sgd_layout (sgd.rs:829-853): one generator seeded `seed`; per node the + end's
// dimensions 1..D-1, then the - end's, each StandardNormal * sqrt(2N); dimension 0 as gfs_init_layout_dim0.
int gfs_init_layout(const gfs_graph_view *g, uint64_t D, uint64_t seed, double *c) {
    if (!g || (!c && g->n_nodes) || D == 0) return fail(GFS_E_ARG, "bad argument");
    Xo256p rng(seed);                                                          // :829
    const double sqrt_n = std::sqrt((double)g->n_nodes * 2.0);                 // :836
    uint64_t len = 0;
    for (uint64_t i = 0; i < g->n_nodes; ++i) {
        c[i * 2 * D + 0] = (double)len;                                        // :839
        for (uint64_t d = 1; d < D; ++d) c[i * 2 * D + d] = standard_normal(rng) * sqrt_n;          // :840-843
        c[i * 2 * D + D] = (double)(len + g->node_len[i]);                     // :846
        for (uint64_t d = 1; d < D; ++d) c[i * 2 * D + D + d] = standard_normal(rng) * sqrt_n;      // :847-850
        len += g->node_len[i];
    }
    return GFS_OK;
}

int gfs_sort_order(const double *x, uint64_t n, uint64_t *order) {         // sgd.rs:665-671
    if ((!x || !order) && n) return fail(GFS_E_ARG, "null argument");
    std::iota(order, order + n, (uint64_t)0);
    // partial_cmp(..).unwrap_or(Equal) + stable sort: ascending, -0.0 == +0.0, ties keep the index
    // order.  NaNs (never produced by a finite run) are placed after all numbers so that the order
    // is total; the device version (gfs_ctx_sort_order) uses the same rule.
    std::stable_sort(order, order + n, [x](uint64_t a, uint64_t b) {
        const double xa = x[a], xb = x[b];
        if (xa != xa) return false;
        if (xb != xb) return true;
        return xa < xb;
    });
    return GFS_OK;
}

// the step-drawing half of calculate_layout_stress (sgd.rs:1218-1250); host only
int gfs_stress_sample_pairs(const gfs_graph_view *g, uint64_t sample_count, uint64_t seed, uint64_t *step_a, uint64_t *step_b,
                            uint64_t *n_out) {
    if (!g || !n_out || ((!step_a || !step_b) && sample_count)) return fail(GFS_E_ARG, "null argument");
    *n_out = 0;
    if (g->n_steps < 2) return GFS_OK;                                     // :1220
    if (!g->path_first_step || g->n_paths == 0 || g->path_first_step[0] != 0 || g->path_first_step[g->n_paths] != g->n_steps)
        return fail(GFS_E_ARG, "path_first_step must start at 0 and end at n_steps");
    for (uint64_t p = 0; p < g->n_paths; ++p)
        if (g->path_first_step[p + 1] < g->path_first_step[p]) return fail(GFS_E_ARG, "path_first_step not monotone");
    Xo256p rng(seed);                                                      // :1218
    uint64_t n = 0;
    for (uint64_t k = 0; k < sample_count; ++k) {
        const uint64_t a = rng.uniform_usize(g->n_steps);                  // :1230
        // the path of step a: the last p with path_first_step[p] <= a (empty paths share a boundary)
        const uint64_t p = (uint64_t)(std::upper_bound(g->path_first_step, g->path_first_step + g->n_paths, a) - g->path_first_step) - 1;
        const uint64_t first = g->path_first_step[p], cnt = g->path_first_step[p + 1] - first;
        if (cnt < 2) continue;                                             // :1234
        const uint64_t rank_a = a - first, rank_b = rng.uniform_usize(cnt);   // :1238-1240
        if (rank_a == rank_b) continue;                                    // :1242
        step_a[n] = first + rank_a; step_b[n] = first + rank_b;
        ++n;
    }
    *n_out = n;
    return GFS_OK;
}

int gfs_batch_plan(const uint64_t *blocks_of_item, uint64_t n, uint64_t max_blocks, uint32_t *launch_of_item, uint32_t *n_launches) {
    if (!n_launches || (n && (!blocks_of_item || !launch_of_item))) return fail(GFS_E_ARG, "null argument");
    const uint64_t bad = gfs::batch_plan(blocks_of_item, n, max_blocks, launch_of_item, n_launches);
    if (bad < n)
        return fail(GFS_E_UNSUPPORTED, "batch item " + std::to_string(bad) + ": its " + std::to_string(blocks_of_item[bad]) +
                                           " workgroups exceed the " + std::to_string(max_blocks) + " of one launch");
    return GFS_OK;
}

}  // extern "C"
