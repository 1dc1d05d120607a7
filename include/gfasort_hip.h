/*
 * gfasort_hip.h — C ABI of libgfasort_hip.so: the MI355X (gfx950) path-guided SGD engine that
 * replaces the inner loops of pangenome/gfasort's `Y` (1D sort) and `L` (nD layout) steps.
 *
 * The reference has no FFI; the seam is the pair of Rust functions
 *     pub fn path_linear_sgd(graph: Arc<BidirectedGraph>, params: PathSGDParams) -> HashMap<usize,f64>
 *                                                                        (src/sgd.rs:237-240)
 *     pub fn path_linear_sgd_layout(graph: Arc<BidirectedGraph>, params: LayoutSGDParams) -> Layout
 *                                                                        (src/sgd.rs:773-776)
 * and this header is what a Rust `extern "C"` block for that seam binds (INTEGRATION.md shows
 * the shim).  Plain pointers and sizes only; caller owns every buffer; nothing is retained
 * after a call returns except inside an explicit gfs_ctx.
 *
 * Return codes: 0 ok; 1 nothing to do (empty graph or no path with >1 step: the reference
 * returns an empty map / zero Layout, sgd.rs:242-244,258-261,780-782,795-798 — leave the graph
 * untouched); <0 error, text in gfs_last_error().  Never throws or aborts across the boundary.
 * There is NO CPU fallback: without a HIP device every compute entry point returns GFS_E_HIP.
 */
#ifndef GFASORT_HIP_H
#define GFASORT_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFS_OK            0
#define GFS_NOTHING_TO_DO 1
#define GFS_E_ARG        (-1)
#define GFS_E_HIP        (-2)
#define GFS_E_NOMEM      (-3)
#define GFS_E_STATE      (-4)
#define GFS_E_UNSUPPORTED (-5)

#define GFS_NO_NODE 0xFFFFFFFFu
#define GFS_MAX_DIMS 8

/* Read-only, caller-owned SoA view of the three things sgd.rs reads from BidirectedGraph
 * (src/graph_ops.rs:10-16): graph.nodes[*].sequence.len(), graph.paths[*].steps and
 * graph.node_order.  Dense node index k = k-th existing node of node_order, i.e. the value
 * the reference stores in handle_to_idx[Handle::forward(id)] (sgd.rs:286-294, 811-814). */
typedef struct gfs_graph_view {
    uint64_t        n_nodes;          /* graph.node_count()                       sgd.rs:241 */
    uint64_t        n_steps;          /* PathIndex::get_total_steps()             sgd.rs:73  */
    uint64_t        n_paths;          /* PathIndex::num_paths()                   sgd.rs:101 */
                                       /* limits of the device mirror: n_nodes < 2^31, n_paths < 2^31,
                                          n_steps <= 2^40, < 2^32 steps and < 2^55 bp per path
                                          (GFS_E_UNSUPPORTED beyond) */
    const uint32_t *node_len;         /* [n_nodes]  sequence.len() by dense index            */
    const uint32_t *step_node;        /* [n_steps]  dense index of the step's node, or
                                         GFS_NO_NODE when the id is absent from the graph
                                         (the reference warns and skips, sgd.rs:525-538)     */
    const uint8_t  *step_is_rev;      /* [n_steps]  Handle::is_reverse()      graph.rs:37    */
    const uint64_t *path_first_step;  /* [n_paths+1] PathInfo.first_step; counts by diff     */
} gfs_graph_view;

/* PathSGDParams, src/sgd.rs:196-212, same field names and order (usize->u64, bool->u8). */
typedef struct gfs_sgd_params {
    uint64_t iter_max;
    uint64_t iter_with_max_learning_rate;
    uint64_t min_term_updates;
    double   delta;                   /* carried, unused — as in the reference               */
    double   eps;
    double   eta_max;
    double   theta;
    uint64_t space;
    uint64_t space_max;
    uint64_t space_quantization_step;
    double   cooling_start;
    uint64_t nthreads;                /* CPU concept; ignored by the HIP engine              */
    uint8_t  progress;
    uint8_t  _pad[7];
    uint64_t seed;
} gfs_sgd_params;

/* LayoutSGDParams, src/sgd.rs:676-707. */
typedef struct gfs_layout_params {
    uint64_t dimensions;              /* 1..GFS_MAX_DIMS                                     */
    gfs_sgd_params sgd;               /* the remaining 14 fields are identical               */
} gfs_layout_params;

/* Device-side launch shape (no reference equivalent; the reference's analogue is nthreads).
 * A "stream" is one Xoshiro256+ generator seeded seed + stream_base + t, exactly what
 * reference worker thread tid = stream_base + t uses (sgd.rs:431-432); one GPU lane owns one
 * stream.  All-zero = defaults. */
typedef struct gfs_launch_config {
    uint64_t n_streams;               /* 0 = auto (fill the chip, >= 1 update per stream)    */
    uint64_t stream_base;             /* first global stream id on this device (multi-GPU)   */
    uint64_t term_updates_per_iteration; /* 0 = params.min_term_updates (this device's share) */
    uint64_t attempt_factor;          /* 0 = 64: a stream gives up an iteration after
                                         attempt_factor*quota+1024 sampled-and-rejected trips */
    uint32_t block_size;              /* 0 = 256                                             */
    uint32_t flags;                   /* GFS_F_*                                             */
    uint64_t trace_per_stream;        /* debug: keep the first k successful terms per stream */
} gfs_launch_config;

#define GFS_F_PLAIN_LOADS   1u        /* read positions with plain (L2-cacheable) loads instead
                                         of agent-scope relaxed atomic loads                 */
#define GFS_F_NO_LDS_TABLES 2u        /* keep zeta/path tables in global memory              */
/* Sampling bundle: n adjacent lanes share ONE sampled (step a, jump) drawn by an ordinary reference
 * stream and take n consecutive steps of the path with the same signed jump (nD: and the same
 * pair of end flips), so that record loads, position loads and atomics of a bundle coalesce into a
 * few 64-B requests (gfasort_amd/csrc/sgd_device.h).  n = 1: reference streams, every lane is a
 * reference worker thread.  n = 0 (default): the library picks — 1 for graphs of < 16384 nodes, else the widest
 * bundle (64, 32, ...) for which >= 95 % of the steps lie in paths of at least 4 n steps (measured basis:
 * profiles/r03/policy_sweep.log).  Layouts of 4..8 dimensions: auto keeps reference streams (n = 1) — their team kernels
 * (n = 8..64) are new and measured on few graphs, and switching would change every existing run's output;
 * an explicit n selects them.  n = 4 is for the 1D sort only.  On graphs whose haplotypes disagree by kilobases the
 * bundled sampler needs a longer schedule than the reference's to reach the same quality (tests/test_gpu_quality.py), or
 * GFS_F_PHASED, which reaches it at the default schedule. */
#define GFS_F_BUNDLE(n) (((uint32_t)(n) & 0xFFu) << 16)  /* n in {0 = auto, 1, 4, 8, 16, 32, 64} */
/* Long runs: with bundles of 64 a sampled (step a, jump) is expanded over k consecutive trips of its wave, i.e. over
 * 64*k consecutive steps (k adapts downwards on short paths).  k = 0 (default): 64 for the 1D sort, 16 for the layout
 * kernels, less where an iteration would otherwise draw fewer than 64 leaders (a leader stands for up to 64 * k * partners
 * terms).  k = 1: a run is one trip. */
#define GFS_F_CHAIN(k) (((uint32_t)(k) & 0xFFu) << 24)   /* k in {0 = auto, 1, 2, 4, 8, 16, 32, 64} */
#define GFS_F_NO_FUSE       4u        /* gfs_ctx_run / gfs_ctx_run_range: one launch per iteration even where
                                         a fused persistent launch is possible                        */
#define GFS_F_ONE_PARTNER   0x10u     /* team kernels at B = 64 (1D; layouts of 2..8 dimensions): one partner draw per leader
                                         (default: two — a sampled step a with two independent draws of its partner b; where
                                         both are line-aligned long jumps the two terms of a lane share the loads and the add
                                         of their a-side) */
/* Phased sampler of the 1D sort (gfs_ctx_setup_1d, gfs_path_linear_sgd, gfs_path_sgd_sort): every iteration outside a window
 * [k_begin, k_end) around the switch to the cooling phase is the team sampler at B = 64; inside it every lane is reference
 * stream `tid` and draws its terms exactly as GFS_F_BUNDLE(1) does.  Both use the same per-lane RNG states, each continuing
 * the state the other left; a team pass left over when the window begins is kept and dropped by the team's own rule (the
 * cooling flag changed) — the oracle's gfo_state with its bundle switched between 64 and 1 between iterations.  n_streams is
 * the team sampler's.  Where the auto policy picks reference streams (graphs of < 16384 nodes) the flag changes nothing.
 * Refused (GFS_E_ARG) with gfs_ctx_setup_nd, with a GFS_F_BUNDLE other than 0 or 64, and with gfs_rank_create.  Default
 * window: gfs_phase_window.  DESIGN.md §3 (K1e) and §5. */
#define GFS_F_PHASED        0x40u
/* Record width of the 1D team kernels' trips at B = 64.  Beside the 16-byte step records a context keeps 8-byte trip records
 * { slot, low position word } (8 B per step more), and the trips read those where nothing is lost by it: every step position of
 * the graph is below 2^32 bp and no node is crowded at the context's stream count (gfasort_amd/csrc/launch_policy.h
 * compact_records).  Same terms, same bits, half the record bytes.  This flag keeps the trips on the 16-byte records. */
#define GFS_F_FULL_RECORDS  0x80u
#define GFS_F_DBG_NO_TWIN_TRIP 0x400u /* diagnostic: the two partners of a leader as two trips even where one would do   */
#define GFS_F_DBG_FREE_RUNNING 0x20u   /* diagnostic: fused launches with a fixed quota per wave and iteration and no pacing
                                         (round 1's launch; the waves drift apart in the schedule) instead of work pools */
#define GFS_F_DBG_NO_ATOMICS 0x100u   /* diagnostic ablation (wrong results): skip the atomic adds */
#define GFS_F_DBG_NO_XLOADS  0x200u   /* diagnostic ablation (wrong results): skip position loads  */
#define GFS_F_DBG_ONE_COLOUR   0x800u  /* diagnostic: short-jump runs execute their first colour only (round-1 behaviour:
                                         half of the run's terms, i.e. short jumps under-sampled)                  */
#define GFS_F_DBG_NO_ALIGN      0x1000u /* diagnostic: bundled sampler without line-aligned runs               */
#define GFS_F_DBG_ALIGN_FIRST   0x2000u /* diagnostic: line-align only the first run of a bundle               */
#define GFS_F_DBG_NO_FUSED_TRIP 0x8000u /* diagnostic: the two colours of a short-jump run as two trips even where one
                                         fused trip is possible (same terms, same order)                        */
#define GFS_F_DBG_WIDE_INDEX 0x4000u  /* test hook: draw step indices with the u64 sampler that graphs of
                                         more than 2^32-1 steps use (rand's usize sampler switches there) */

typedef struct gfs_stats {
    uint64_t term_updates;            /* successful updates, counted where sgd.rs:579 counts */
    uint64_t attempts;                /* loop trips including `continue`s                    */
    uint64_t iterations;              /* batches launched                                    */
    uint64_t n_streams;               /* streams actually used                               */
    uint64_t bundle;                  /* lanes per sampling bundle actually used (1 = reference streams) */
    double   kernel_ms;               /* sum of SGD kernel durations (HIP events)            */
    double   total_ms;                /* wall time inside the call (one-shot) / run          */
    uint64_t launches;                /* SGD kernel launches (a fused launch covers many iterations) */
    uint64_t run_trips;               /* longest run in trips (GFS_F_CHAIN) actually used; 1 = one trip per run */
} gfs_stats;

/* One sampled term (debug trace): 1D i,j = dense node index; nD = 2*idx+end. */
typedef struct gfs_term {
    uint32_t i, j;
    double   d_ij;
} gfs_term;

typedef struct gfs_ctx gfs_ctx;

/* ---- library ---- */
const char *gfs_version(void);
const char *gfs_last_error(void);
int         gfs_device_count(void);
/* optional: create the HIP context now (e.g. on a side thread while the caller parses its input) */
int         gfs_warmup(int device);

/* ---- host tables, bit-exact restatements (no device needed) ---- */
/* fast_precise_pow                                                        sgd.rs:155-182 */
double   gfs_fast_precise_pow(double a, double b);
/* path_linear_sgd_schedule with w_min=1/eta_max, w_max=1: etas[iter_max+1]  sgd.rs:300-308,617-638 */
int      gfs_sgd_schedule(const gfs_sgd_params *p, double *etas);
/* zeta table length and contents                                          sgd.rs:311-331 */
uint64_t gfs_zeta_table_len(const gfs_sgd_params *p);
int      gfs_zeta_table(const gfs_sgd_params *p, double *zetas);
/* initial positions x[idx] = bp prefix in node_order                      sgd.rs:271-294 */
int      gfs_init_positions(const gfs_graph_view *g, double *x);
/* layout init, dimension 0 only (+end = prefix, -end = prefix+len), Layout order; the
 * Gaussian dimensions >=1 (rand_distr StandardNormal, sgd.rs:829-850): gfs_init_layout, or the caller's.   */
int      gfs_init_layout_dim0(const gfs_graph_view *g, uint64_t dims, double *coords);
/* the reference's whole layout start (sgd.rs:829-853): dimension 0 as above, dimensions >= 1 = StandardNormal * sqrt(2N)
 * from ONE Xoshiro256+ seeded `seed`, drawn node by node (+ end, then - end).  rand_distr's ziggurat is restated from
 * its published algorithm with rebuilt tables: parity unpinned.                                       */
int      gfs_init_layout(const gfs_graph_view *g, uint64_t dims, uint64_t seed, double *coords);
/* positions -> rank order (ascending, ties by dense index)                sgd.rs:665-671 */
int      gfs_sort_order(const double *x, uint64_t n, uint64_t *order);

/* ---- one-shot entry points: what the Rust seam functions bind ---- */
/* replaces path_linear_sgd (src/sgd.rs:237).  x_inout[n_nodes]: in = initial positions
 * (NULL-initialised by gfs_init_positions if init_x != 0), out = final positions.
 * etas / zetas may be NULL (computed as the reference does).                               */
int gfs_path_linear_sgd(const gfs_graph_view *g, const gfs_sgd_params *p,
                        const gfs_launch_config *cfg, const double *etas, const double *zetas,
                        int init_x, double *x_inout, gfs_stats *stats);
/* replaces path_sgd_sort (src/sgd.rs:641): the same run, plus order_out[r] = dense index of the node
 * of rank r (ascending position, ties by dense index; sorted on the device).  x_inout as above.   */
int gfs_path_sgd_sort(const gfs_graph_view *g, const gfs_sgd_params *p,
                      const gfs_launch_config *cfg, const double *etas, const double *zetas,
                      int init_x, double *x_inout, uint64_t *order_out, gfs_stats *stats);
/* replaces path_linear_sgd_layout (src/sgd.rs:773).  coords_inout[n_nodes*2*D] in the order of
 * Layout.coords: coords[node*2*D + end*D + dim] (src/layout.rs:14,73-78).                   */
int gfs_path_linear_sgd_layout(const gfs_graph_view *g, const gfs_layout_params *p,
                               const gfs_launch_config *cfg, const double *etas, const double *zetas,
                               double *coords_inout, gfs_stats *stats);

/* ---- resident API: graph and positions stay in HBM between calls ---- */
int   gfs_ctx_create(const gfs_graph_view *g, int device, gfs_ctx **out);
/* Same, with an explicit internal node layout: node_perm[k] = slot of dense node k in the device
 * position vector (a permutation of 0..n_nodes-1).  NULL = first-visit path order with branches placed where they branch off (the default of
 * gfs_ctx_create).  Ranks of a multi-GPU run that all-reduce the device buffer in place must share
 * one layout.  Upload / download / trace always speak the ABI's dense indices and Layout.coords order;
 * only the raw device pointer (gfs_ctx_positions_device / gfs_ctx_bind_positions) is in device order:
 * 1D x[slot]; nD the end x dimension planes coords[end][dim][slot] (element-wise collectives do not care). */
int   gfs_ctx_create_with_layout(const gfs_graph_view *g, int device, const uint32_t *node_perm, gfs_ctx **out);
int   gfs_ctx_node_layout(const gfs_ctx *ctx, uint32_t *perm_out, uint64_t n_nodes);
void  gfs_ctx_destroy(gfs_ctx *ctx);
int   gfs_ctx_setup_1d(gfs_ctx *ctx, const gfs_sgd_params *p, const gfs_launch_config *cfg,
                       const double *etas, const double *zetas);
int   gfs_ctx_setup_nd(gfs_ctx *ctx, const gfs_layout_params *p, const gfs_launch_config *cfg,
                       const double *etas, const double *zetas);
uint64_t gfs_ctx_positions_len(const gfs_ctx *ctx);              /* n_nodes (1D) or n_nodes*2*D */
int   gfs_ctx_upload_positions(gfs_ctx *ctx, const double *host, uint64_t n);
int   gfs_ctx_init_positions(gfs_ctx *ctx);                      /* 1D: the reference's start (sgd.rs:286-294),
                                                                    prefix sum of node lengths, on the device */
int   gfs_ctx_download_positions(gfs_ctx *ctx, double *host, uint64_t n);
void *gfs_ctx_positions_device(gfs_ctx *ctx);                    /* device pointer (for RCCL)   */
int   gfs_ctx_bind_positions(gfs_ctx *ctx, void *device_ptr);    /* use a caller-owned buffer   */
int   gfs_ctx_reset_streams(gfs_ctx *ctx);                       /* re-seed RNG streams, zero stats */
/* one SGD batch: iteration k in 0..=iter_max uses etas[k]; cooling for
 * k > floor(cooling_start*iter_max) (sgd.rs:297,383-396).  Asynchronous on hip_stream
 * (a hipStream_t, NULL = the default stream).                                               */
int   gfs_ctx_run_iteration(gfs_ctx *ctx, uint64_t k, void *hip_stream);
/* GFS_F_PHASED's default window [*k_begin, *k_end) for these parameters (host only): around first_cooling =
 * floor(cooling_start * iter_max), scaled with iter_max; always k_begin <= k_end <= iter_max + 1. */
int   gfs_phase_window(const gfs_sgd_params *p, uint64_t *k_begin, uint64_t *k_end);
/* iterations ks[0..n): ONE fused persistent launch (the team kernels at their widest bundle: sorts, layouts of 2..8
 * dimensions; reference streams in any dimension) in which the waves walk the schedule and draw every iteration's exact
 * number of updates from a shared pool; otherwise (narrower bundles, traces, GFS_F_NO_FUSE, more streams than fit on the
 * device at once, an iteration of >= 2^31 updates per pool counter) n launches.  A range of ONE layout iteration is pooled
 * as well where it is many chunks per wave (gfs_ctx_run_iteration keeps a fixed quota per wave).  Asynchronous.         */
int   gfs_ctx_run_range(gfs_ctx *ctx, const uint64_t *ks, uint64_t n, void *hip_stream);
int   gfs_ctx_run(gfs_ctx *ctx, void *hip_stream);               /* k = 0..=iter_max (run_range), then sync */
int   gfs_ctx_synchronize(gfs_ctx *ctx, void *hip_stream);
int   gfs_ctx_stats(gfs_ctx *ctx, gfs_stats *out);               /* synchronises                */
/* rank order of the context's current 1D positions, sorted on the device (rocPRIM radix sort)   */
int   gfs_ctx_sort_order(gfs_ctx *ctx, uint64_t *order, uint64_t n_nodes);
int   gfs_ctx_trace(gfs_ctx *ctx, gfs_term *out, uint64_t n_terms, uint64_t *counts, uint64_t n_streams);
/* ---- test hooks (not part of the integration surface) ----
 * the n_steps + 1 16-byte step records (the last one is the zeroed padding record) as 4 u32 words each;
 * n_words must be 4 * (n_steps + 1) */
int   gfs_ctx_debug_step_records(const gfs_ctx *ctx, uint32_t *out, uint64_t n_words);
/* crowding onset: set >= 0 overrides the kshift of every later launch of this context, set = -1 restores the policy,
 * set < -1 changes nothing; *kshift_out (nullable) receives the value the kernels are handed (the context must be set up) */
int   gfs_ctx_debug_kshift(gfs_ctx *ctx, int32_t set, int32_t *kshift_out);
/* Bytes of the per-step record the trips of this context's next launch read: 8 (trip records) or 16 (step records; every kernel
 * but the 1D team kernels at B = 64, GFS_F_FULL_RECORDS, a graph that is not eligible).  0: the context is not set up or has no
 * work.  Follows gfs_ctx_debug_kshift.  The 8-byte records are made when a context is created (not for the items of a context
 * set) and given up for good by gfs_ctx_setup_nd.  A batch (gfs_batch_*) takes reference-stream contexts only: always 16. */
uint32_t gfs_ctx_record_bytes(const gfs_ctx *ctx);
/* GFS_F_PHASED's window: set_begin, set_end >= 0 replace it for later launches (0 <= begin <= end <= iter_max + 1, else
 * GFS_E_ARG), both < 0 only query; *begin_out / *end_out (nullable) receive the effective window — the whole schedule where the
 * flag is a no-op (reference streams picked), on which a window cannot be set (GFS_E_STATE).  GFS_E_STATE on a context not set
 * up with the flag. */
int   gfs_ctx_phase_window(gfs_ctx *ctx, int64_t set_begin, int64_t set_end, uint64_t *begin_out, uint64_t *end_out);

/* ---- quality read-outs (K7): how good is what is in HBM now ----
 * Every entry evaluates ONE per-pair formula, the reference's (calculate_layout_stress, sgd.rs:1252-1275, Layout::distance):
 *   d_path = |(double)pos_a - (double)pos_b|, d_layout = sqrt(sum over dimensions, left to right, of (c_a - c_b)^2) between the
 *   + ends of the two steps' nodes (1D: one term), err = d_layout - d_path, rel_sq = err*err / (d_path*d_path);
 * a pair is skipped when d_path == 0, when either step's node is absent, or when the steps lie in different paths.  A pair's
 * value is the reference's bit for bit.  The kernels write nothing but their own output: positions, records and RNG streams
 * are left alone, so a read-out between two gfs_ctx_run_range calls does not change the run.  Results are deterministic and do
 * not depend on the device: the launch shape is a function of n_steps, every reduction has a fixed order, no float atomics.
 * On a rank's context (gfs_rank_ctx) a read-out covers that rank's shard of the paths, on that rank's replica. */
typedef struct gfs_pair_error {
    uint64_t step_distance;           /* z: pairs of steps (s, s + z) of one path                                   */
    uint64_t pairs;                   /* pairs not skipped                                                          */
    double   sum_rel_sq;              /* sum of rel_sq: rms relative error = sqrt(sum_rel_sq / pairs)               */
    double   max_rel_sq;              /* exact (order-independent)                                                  */
    double   sum_abs;                 /* sum of |err|, bp                                                           */
    double   sum_sq;                  /* sum of err^2, bp^2                                                         */
} gfs_pair_error;

/* measure_layout_quality.rs:100-208 on the graph SORTED by the context's current 1D positions: a node's position is the prefix
 * sum of node lengths in rank order; per pair of consecutive path steps the genomic distance is the first node's length and
 * the layout distance |pos_b - pos_a|; a pair whose first node is absent is skipped, an absent second node counts as
 * position 0.  mae = abs_err_sum / steps, rmse = sqrt(sq_err_sum / steps), relative_error = abs_err_sum / genomic_sum. */
typedef struct gfs_sort_quality {
    uint64_t steps;                   /* pairs counted                                                              */
    uint64_t abs_err_sum;             /* exact                                                                      */
    uint64_t genomic_sum;             /* exact                                                                      */
    double   sq_err_sum;              /* every term exact, summed in a fixed order                                  */
} gfs_sort_quality;

/* all pairs (s, s + z) for each z = zs[0..n_z) (n_z <= 65535) in one launch on hip_stream; synchronises before returning.
 * out[n_z].  GFS_E_ARG (before any device call) for null pointers or a z of 0, GFS_E_STATE on a context without positions.
 * A z no path is long enough for gives pairs = 0 and zero sums. */
int gfs_ctx_pair_errors(gfs_ctx *ctx, const uint64_t *zs, uint64_t n_z, gfs_pair_error *out, void *hip_stream);
/* host only: the sample stream of calculate_layout_stress (sgd.rs:1218-1250) — one Xoshiro256+ seeded `seed` (the reference's is
 * 12345), step a uniform over all steps, rank b uniform over its path, in the reference's draw order — less the candidates its
 * data-independent `continue`s drop (paths of fewer than 2 steps, rank_a == rank_b).  step_a, step_b: [sample_count]; *n_out
 * pairs are written.  A graph of fewer than 2 steps gives none (:1220). */
int gfs_stress_sample_pairs(const gfs_graph_view *g, uint64_t sample_count, uint64_t seed, uint64_t *step_a, uint64_t *step_b,
                            uint64_t *n_out);
/* rel_sq of the pairs (step_a[i], step_b[i]), i < n, on the device; rel_sq_out (nullable, [n]) receives them, a skipped pair as
 * -1.  *counted = pairs not skipped, *stress = sqrt(sum of rel_sq / counted) with the sum taken on the host in the order of
 * the list — on gfs_stress_sample_pairs' list the reference's calculate_layout_stress bit for bit — or 0.0 where nothing was
 * counted.  GFS_E_ARG for a step >= n_steps.  Synchronises. */
int gfs_ctx_stress_of_pairs(gfs_ctx *ctx, const uint64_t *step_a, const uint64_t *step_b, uint64_t n, double *rel_sq_out /*nullable*/,
                            uint64_t *counted, double *stress);
/* 1D contexts only (GFS_E_STATE otherwise); the order is gfs_ctx_sort_order's.  GFS_E_UNSUPPORTED for a graph of 2^53 bp or more. */
int gfs_ctx_sort_quality(gfs_ctx *ctx, gfs_sort_quality *out);
/* one-shot, for a caller that holds a finished result and no context: builds a context on device 0, uploads, measures.
 * dims = 0: positions is x[n_nodes] by dense index; dims = 1..GFS_MAX_DIMS: Layout.coords order, n_nodes*2*dims. */
int gfs_pair_errors(const gfs_graph_view *g, uint64_t dims, const double *positions, const uint64_t *zs, uint64_t n_z,
                    gfs_pair_error *out);
/* one-shot, as gfs_pair_errors is for K7a: builds a context on device 0, uploads x[n_nodes] by dense index, measures.  (gfs_sort_quality
 * is the result's type, so the entry is gfs_sort_quality_of.) */
int gfs_sort_quality_of(const gfs_graph_view *g, const double *positions, gfs_sort_quality *out);

/* ---- where the error sits (K7d, K7e, K7f): per path, per pair, per node, at ONE step distance z ----
 * The pairs, the per-pair formula and its skips are those above.  With d_layout = err + d_path, a counted pair is STRETCHED when
 * d_layout / d_path > ratio (one double division, one comparison); the reference's diagnostic binary (src/bin/sgd_diagnostics.rs)
 * lists the stretched pairs at z = 1, ratio = 10 and counts each path's reverse steps.  Two departures from that binary:
 *   - it measures positions that are prefix sums of node lengths in node-id order; these entries measure whatever the context
 *     holds — after gfs_ctx_init_positions on a graph whose nodes are in id order that is the same thing;
 *   - it gives a node it cannot find position 0; here the pair is skipped, as everywhere in K7.
 * Same rules as above: nothing but the outputs is written, every figure is a function of graph, z, ratio and positions alone
 * (the step table is cut into tiles of a constant number of steps, a tile is reduced by a fixed tree, a path's tiles are
 * combined in tile order; per node only integer sums and a maximum are accumulated, which no order of arrival changes).
 * GFS_E_ARG (before any device call) for a null pointer, z == 0, a ratio that is NaN or negative, or a length that does not match
 * the context; GFS_E_STATE on a context without positions.  A z no path is long enough for gives zero figures and *total = 0.
 * All entries run on hip_stream and synchronise before returning.  On a rank's context (gfs_rank_ctx): the rank's shard, in the
 * shard's path numbering. */
typedef struct gfs_path_error {
    uint64_t steps;                   /* steps of the path                                                          */
    uint64_t reverse_steps;           /* of which reverse                                                           */
    uint64_t pairs;                   /* pairs (s, s + z) of the path not skipped                                   */
    double   sum_rel_sq;              /* as gfs_pair_error, over this path's pairs                                  */
    double   max_rel_sq;              /* exact                                                                      */
    double   sum_abs;
    double   sum_sq;
    uint64_t stretched;               /* counted pairs with d_layout / d_path > ratio                               */
} gfs_path_error;

typedef struct gfs_stretched_pair {
    uint64_t step_a, step_b;          /* step_b = step_a + z                                                        */
    uint64_t path;
    double   d_path, d_layout;
} gfs_stretched_pair;

typedef struct gfs_node_error {
    uint64_t pairs;                   /* counted pairs with the node at either end; both ends on it: counted once   */
    uint64_t stretched;               /* of which stretched                                                         */
    double   max_rel_sq;              /* largest rel_sq of those pairs, exact                                       */
} gfs_node_error;

/* out[n_paths], by path index; n_paths must be the context's */
int gfs_ctx_path_errors(gfs_ctx *ctx, uint64_t z, double ratio, gfs_path_error *out, uint64_t n_paths, void *hip_stream);
/* the stretched pairs in ascending step_a: *total receives their exact number, out[0 .. min(cap, *total)) the first of them;
 * entries beyond are left untouched.  out may be NULL when cap = 0.  The listed prefix is the same on every call. */
int gfs_ctx_stretched_pairs(gfs_ctx *ctx, uint64_t z, double ratio, gfs_stretched_pair *out, uint64_t cap, uint64_t *total,
                            void *hip_stream);
/* out[n_nodes], by dense node index; n_nodes must be the context's */
int gfs_ctx_node_errors(gfs_ctx *ctx, uint64_t z, double ratio, gfs_node_error *out, uint64_t n_nodes, void *hip_stream);
/* one-shot, as gfs_pair_errors: paths_out[g->n_paths], pairs_out[cap] (NULL when cap = 0), *total */
int gfs_diagnose(const gfs_graph_view *g, uint64_t dims, const double *positions, uint64_t z, double ratio,
                 gfs_path_error *paths_out, gfs_stretched_pair *pairs_out, uint64_t cap, uint64_t *total);

/* ---- batches: many small graphs in one persistent launch (no reference equivalent) ----
 * A graph of fewer than 16384 nodes runs reference streams, at most one per 4 nodes: a few workgroups on a chip of hundreds of
 * CUs.  A batch runs the whole schedule of many configured contexts in one launch whose grid is the concatenation of theirs; every
 * workgroup works on its own context's buffers exactly as a launch of that context alone does.  After gfs_batch_run each context
 * is as if gfs_ctx_run had run it alone — positions, RNG streams and counters advanced, iterations += iter_max + 1, launches += 1 —
 * so gfs_ctx_download_positions, gfs_ctx_sort_order, the quality read-outs and gfs_ctx_stats work per item; one stream per item is
 * bit for bit the solo run.  A context's kernel_ms is NOT advanced by a batch: the time belongs to the batch (gfs_batch_stats).
 * Running a batch again continues every item's streams, as a second gfs_ctx_run does.
 * A batch BORROWS its contexts: they must outlive it and must not be set up again while it exists (gfs_batch_run returns
 * GFS_E_STATE, naming the item, where a context's workgroups, iterations, LDS use or plan are no longer those the batch's launches
 * were cut for).  All items: one device; one
 * kind (all 1D sorts, or all layouts of the same 2 or 3 dimensions); set up so that their plan is the pooled fused reference-stream
 * kernel (bundle 1 — chosen or GFS_F_BUNDLE(1) —, no trace, no GFS_F_NO_FUSE, no GFS_F_PHASED window in effect); one block size;
 * iter_max + 1 <= 4096.  Otherwise GFS_E_UNSUPPORTED; GFS_E_ARG for null, n == 0 or the same context twice; GFS_E_STATE for a
 * context that is not set up; the text names the item; these checks come before any device call.  Items keep their own parameters,
 * schedules (iter_max may differ), quotas, seeds and stream counts.  A context with nothing to do is skipped and left alone.
 * Items with and without LDS tables go into separate launches; a launch's dynamic LDS is the largest among its items.
 * Either side of the run, a batch of 1D sorts does for all its items at once what gfs_ctx_init_positions, gfs_ctx_download_positions
 * and gfs_ctx_sort_order do for one: gfs_batch_init_positions, one launch; gfs_batch_results, one launch per
 * padded segment length and two copies, a workgroup sorting its item's (key, dense index) pairs in LDS.  Items of more than
 * GFS_SEGMENT_SORT_CAP nodes take the per-context sort, once each, into the same arrays: no item is refused for its size.  Items
 * with nothing to do are covered like the others.  The read-out changes no item's positions, RNG streams or counters.
 * A batch of layouts is fed and read the same way (K4c / K6c): gfs_batch_upload_coords and gfs_batch_coords move every item's
 * coordinates as one packed array, one launch and one copy each; gfs_batch_init_positions and gfs_batch_results stay the sorts'
 * and refuse layouts.  Either kind reads every item's gfs_ctx_pair_errors in one call, gfs_batch_pair_errors (K7g). */
#define GFS_SEGMENT_SORT_CAP 8192      /* nodes of the largest item sorted in LDS (96 KiB of a CU's 160) */
typedef struct gfs_batch gfs_batch;
typedef struct gfs_batch_config {
    uint64_t max_blocks_per_launch;   /* 0 = what the device holds at once (occupancy of the batch kernel at the launch's
                                         block size and largest LDS table, times the CU count); a smaller value is a test
                                         hook and a way to leave room for other work */
    uint64_t reserved[3];
} gfs_batch_config;
typedef struct gfs_batch_stats {
    uint64_t items, items_run;        /* contexts given / contexts that had something to do */
    uint64_t launches;
    uint64_t blocks;                  /* workgroups over all launches */
    uint64_t term_updates, attempts;  /* sums over the items, from their own counters */
    double   kernel_ms, total_ms;     /* HIP events around the batch launches / wall time inside gfs_batch_run */
} gfs_batch_stats;

/* host only, no device: items in the given order, a new launch where the next item would not fit (an exact fit is taken); an item
 * never straddles two launches.  launch_of_item[n]; *n_launches.  GFS_E_UNSUPPORTED if one item alone exceeds max_blocks.
 * gfs_batch_create cuts its launches with it, so that every workgroup of a launch is resident at once: a graph whose
 * workgroups start late drifts in its schedule. */
int  gfs_batch_plan(const uint64_t *blocks_of_item, uint64_t n, uint64_t max_blocks, uint32_t *launch_of_item, uint32_t *n_launches);
int  gfs_batch_create(gfs_ctx *const *ctxs, uint64_t n, const gfs_batch_config *cfg /*nullable*/, gfs_batch **out);
int  gfs_batch_run(gfs_batch *b, void *hip_stream);      /* every item's k = 0..=iter_max, then synchronises */
int  gfs_batch_get_stats(gfs_batch *b, gfs_batch_stats *out);   /* synchronises */
void gfs_batch_destroy(gfs_batch *b);
/* host only: offsets[i] = sum of n_nodes of items 0..i-1, in the order given to gfs_batch_create (idle items included);
 * offsets[items] = total.  n must be items + 1. */
int  gfs_batch_result_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n);
/* gfs_ctx_init_positions on every item, in one launch; then synchronises */
int  gfs_batch_init_positions(gfs_batch *b, void *hip_stream);
/* every item's positions (dense order, as gfs_ctx_download_positions) and rank order (as gfs_ctx_sort_order, as uint32_t)
 * at offsets[i]; either pointer may be NULL; total must be offsets[items]; *kernel_ms (nullable): HIP events around the
 * read-out launches; synchronises.  GFS_E_ARG for a null batch, both pointers NULL or a wrong total; GFS_E_UNSUPPORTED for a batch
 * of layouts (both calls); an item on which gfs_ctx_sort_order would fail fails the call with that code, the text naming the item;
 * all checked before any device call. */
int  gfs_batch_results(gfs_batch *b, double *positions, uint32_t *order, uint64_t total, double *kernel_ms, void *hip_stream);
/* test hook: items of more than cap nodes take the per-item sort (0 restores GFS_SEGMENT_SORT_CAP; larger values are GFS_E_ARG) */
int  gfs_batch_debug_sort_cap(gfs_batch *b, uint64_t cap);
/* A batch of layouts (D = 2 or 3): every item's coordinates in one packed array, Layout.coords order (k*2 + end)*D + dim by dense index k,
 * item i at offsets[i] * 2 * D (gfs_batch_result_offsets); total must be offsets[items] * 2 * D.  Up: one copy through the batch's pinned
 * staging and one launch write every item's end x dimension planes by node slot, exactly what gfs_ctx_upload_positions writes; down: one
 * launch and one copy give every item the bits of gfs_ctx_download_positions; *kernel_ms (nullable): HIP events around the launch.  Both
 * synchronise.  GFS_E_ARG for a null pointer or a wrong total, GFS_E_UNSUPPORTED for a batch of 1D sorts (gfs_batch_init_positions and
 * gfs_batch_results are theirs), GFS_E_STATE, naming the item, for a context no longer set up for the batch's dimensions; all checked
 * before any device call.  Items with nothing to do are covered like the others; no RNG stream or counter is touched. */
int  gfs_batch_upload_coords(gfs_batch *b, const double *coords, uint64_t total, void *hip_stream);
int  gfs_batch_coords(gfs_batch *b, double *coords, uint64_t total, double *kernel_ms /*nullable*/, void *hip_stream);
/* gfs_ctx_pair_errors of every item, for sorts and layouts alike: out[i * n_z + k] is item i at zs[k], field for field and bit for
 * bit what the item's own call gives (a workgroup of the one step launch does the work of a workgroup of the item's own launch;
 * an item's partial sums are added in the same order).  One step launch and one reduce launch over all items and distances,
 * one copy back; scratch is the batch's.  Arguments as gfs_ctx_pair_errors (GFS_E_ARG for a null pointer with n_z > 0, a
 * distance of 0, more than 65535 distances), GFS_E_STATE, naming the item, for a context without positions; checked before any
 * device call.  *kernel_ms (nullable): HIP events around the two launches.  Runs on hip_stream and synchronises; writes nothing
 * but out. */
int  gfs_batch_pair_errors(gfs_batch *b, const uint64_t *zs, uint64_t n_z, gfs_pair_error *out /*[items][n_z]*/, double *kernel_ms /*nullable*/,
                           void *hip_stream);
/* The diagnosis of every item, for sorts and layouts alike, one step distance z and one ratio for the whole batch (DESIGN.md §3,
 * K7h / K7i / K7j): what gfs_ctx_path_errors, gfs_ctx_stretched_pairs and gfs_ctx_node_errors give one item at a time, field for
 * field and the doubles bit for bit (a tile of 512 steps yields the same whoever runs it, a path's tiles are folded in tile order,
 * per node only integer sums and a maximum are accumulated), in a number of launches that does not depend on the number of items:
 * paths 2 launches; pairs 2 launches, a memset and one scan; nodes 2 launches and a memset.  Tables go up in one copy through the
 * batch's pinned staging, results come back in one; scratch is the batch's, nothing is allocated per call once it has grown.
 *   gfs_batch_path_offsets   host only: offsets[i] = sum of n_paths of items 0..i-1, offsets[items] = total_paths; n = items + 1
 *   gfs_batch_path_errors    out[offsets[i] + p] = path p of item i; total_paths must be offsets[items]
 *   gfs_batch_stretched_pairs  totals[i] = item i's exact number of stretched pairs; out[i * cap + k], k < min(cap, totals[i]), its
 *                            first pairs in ascending step_a, step and path numbers the item's own; entries past that are left
 *                            untouched; out may be NULL when cap = 0.  The cap is applied on the device: one synchronise
 *   gfs_batch_node_errors    out[offsets[i] + k] = dense node k of item i, offsets those of gfs_batch_result_offsets; total_nodes
 *                            must be offsets[items]
 * GFS_E_ARG for a null batch or pointer, z == 0, a ratio that is NaN or negative, or a wrong total (gfs_ctx_*'s rules); GFS_E_STATE,
 * naming the item, for a context without positions or no longer of the batch's dimensions; all checked before any device call and
 * before anything is written.  *kernel_ms (nullable): HIP events around the launches.  Every entry runs on hip_stream and
 * synchronises; nothing but the outputs is written: positions, RNG streams and counters are untouched. */
int  gfs_batch_path_offsets(const gfs_batch *b, uint64_t *offsets, uint64_t n);
int  gfs_batch_path_errors(gfs_batch *b, uint64_t z, double ratio, gfs_path_error *out, uint64_t total_paths, double *kernel_ms /*nullable*/,
                           void *hip_stream);
int  gfs_batch_stretched_pairs(gfs_batch *b, uint64_t z, double ratio, gfs_stretched_pair *out /*[items][cap], NULL when cap = 0*/, uint64_t cap,
                               uint64_t *totals /*[items]*/, double *kernel_ms /*nullable*/, void *hip_stream);
int  gfs_batch_node_errors(gfs_batch *b, uint64_t z, double ratio, gfs_node_error *out, uint64_t total_nodes, double *kernel_ms /*nullable*/,
                           void *hip_stream);
/* test hook: caps the grids over flat tiles and paths of K7h and K7i at max_blocks workgroups; 0 restores the default.  No result changes. */
int  gfs_batch_debug_tile_blocks(gfs_batch *b, uint64_t max_blocks);

/* ---- the sort quality of every item (K7k): gfs_ctx_sort_quality of a whole batch of 1D sorts in one call ----
 * One launch per padded segment length present (at most 8), one step launch and one reduce launch, whatever the number of items;
 * an item of more than GFS_SEGMENT_SORT_CAP nodes takes gfs_ctx_sort_quality's own sort and scan once.  The inputs go up in one
 * copy from the batch's pinned staging, the results come back in one; nothing is allocated per call once the scratch has grown.
 * GFS_E_ARG for a null batch or out, or n != the batch's items; GFS_E_UNSUPPORTED for a batch of layouts; GFS_E_STATE, naming the
 * item, for an item that is not a set-up 1D context — all before any device call; GFS_E_UNSUPPORTED, naming the item, for an item
 * of 2^53 bp or more (its length comes back with the results).  out is written only where the call succeeds.  An item without
 * nodes or with fewer than two steps gives a row of zeros.  Synchronises; nothing but the output is written: positions, RNG
 * streams and counters are untouched. */
/* gfs_ctx_sort_quality of every item of a batch of 1D sorts, bit for bit; out[n], n = the batch's items. */
int  gfs_batch_sort_quality(gfs_batch *b, gfs_sort_quality *out, uint64_t n, double *kernel_ms /*nullable*/, void *hip_stream);

/* ---- context sets: the contexts of many small graphs built in one pass ----
 * gfs_ctx_create costs about the same however small the graph is: a score of allocations, six blocking uploads, three sorts, a scan
 * and up to 80 fixpoint rounds with a read-back each.  gfs_ctx_set_create builds n contexts from n views in ONE pass over their
 * disjoint union — one arena for all index arrays, one scratch allocation, one pinned staging buffer; one packed copy up for the
 * steps, path starts, orientations and the item table and one for the node lengths; one scan, two sorts and two fixpoints over the
 * union; one copy of all node layouts back — so that allocations, copies and launches do not grow with n.  Everything the build
 * computes is integer arithmetic, so item i holds, bit for bit, what gfs_ctx_create(graphs[i], device, &c) gives: step records
 * (padding record included), path records, path lengths, node layout and the host-side facts.  Every entry that takes a gfs_ctx
 * takes an item: setup, runs, upload and download, the read-outs, gfs_batch_create, the debug hooks.
 * Ownership: the items belong to the set.  Their index arrays are borrowed from the set's arena; what gfs_ctx_setup_* allocates is
 * each item's own and goes with it.  gfs_ctx_destroy on an item does nothing; gfs_ctx_set_destroy destroys every item.  The set
 * must outlive any gfs_batch made from its items.
 * Errors: gfs_ctx_create's, per item, with a text that begins "set item <i>: " and names the lowest failing item — first the
 * checks that read only counts (with them GFS_E_UNSUPPORTED where the items TOGETHER pass one context's limits: 2^31-1 nodes,
 * 2^31-1 paths, 2^40 steps), then those that read path_first_step, all before any device call; a step naming a node its item does
 * not have is found on the device and gives GFS_E_ARG naming the lowest such item — also in an item of 0 nodes, the one case in
 * which a set differs from gfs_ctx_create, which does not look at the steps of a graph without nodes.  GFS_E_ARG for null
 * arguments or n == 0.  On any failure *out is NULL and nothing stays allocated.  There is no node_perm variant. */
typedef struct gfs_ctx_set gfs_ctx_set;
typedef struct gfs_ctx_set_info {
    uint64_t items, total_nodes, total_steps, total_paths;
    uint64_t launches;            /* of the build: the library's own kernel launches and hipMemsets, counted one by one, plus ONE per
                                     rocPRIM call (two sorts, one scan: how many kernels each launches is rocPRIM's business and depends
                                     on the size).  Fixpoint rounds go out four at a time, so the count steps with the longest chain of
                                     any item, not with the number of items. */
    uint64_t device_allocations;  /* hipMalloc + hipHostMalloc calls of the build */
    uint64_t arena_bytes;         /* the one allocation the items' index arrays live in */
    double   build_ms;            /* wall time inside gfs_ctx_set_create */
} gfs_ctx_set_info;

/* host only, no device: where item i's five index arrays lie in the arena — offsets[5 * i + k] bytes from its start, k = 0 step
 * records (n_steps[i] + 1 of 16 B), 1 path records (16 B), 2 path lengths (8 B), 3 node layout (4 B), 4 node lengths (4 B); arrays
 * of a kind are adjacent, every array starts 256-byte aligned, none overlap.  gfs_ctx_set_create lays its arena out with it. */
int      gfs_ctx_set_plan(const uint64_t *n_nodes, const uint64_t *n_steps, const uint64_t *n_paths, uint64_t n,
                          uint64_t *offsets /*[5*n]: step_rec, path_rec, path_len, perm, node_len*/, uint64_t *arena_bytes);
int      gfs_ctx_set_create(const gfs_graph_view *const *graphs, uint64_t n, int device, gfs_ctx_set **out);
uint64_t gfs_ctx_set_size(const gfs_ctx_set *s);
gfs_ctx *gfs_ctx_set_item(gfs_ctx_set *s, uint64_t i);      /* owned by the set; NULL past the end */
int      gfs_ctx_set_get_info(const gfs_ctx_set *s, gfs_ctx_set_info *out);
void     gfs_ctx_set_destroy(gfs_ctx_set *s);               /* destroys every item */

/* ---- set setup: every item of a context set set up in one pass ----
 * gfs_ctx_setup_* costs five to eight allocations, two blocking memsets and three blocking copies per context, and computes a zeta
 * table and seeds every RNG stream on the host.  gfs_ctx_set_setup_1d / _nd set up ALL items of a set in one pass: the state arrays
 * of every item in ONE arena the set owns (laid out by gfs_ctx_set_state_plan), one memset over everything a setup zeroes, every
 * zeta table, schedule table and the seeding kernel's tables in ONE pinned staging buffer and up in one copy, every RNG stream
 * seeded by ONE launch (set_seed_streams_kernel) — so that allocations, copies and launches do not depend on the number of items.
 * Items that share theta, space_max and space_quantization_step get slices of one zeta running sum.
 * Contract: item i then holds, bit for bit, what gfs_ctx_setup_1d(item, &params[i], &cfgs[i], NULL, NULL) (or _nd) would have left:
 * shape, plan, parameters, schedule, the RNG words, the zeta table with its zero padding, the schedule table, zeroed counters,
 * positions, team state and trace buffers.  Every launch shape the single call accepts is accepted (team kernels, GFS_F_PHASED,
 * tracing).  There is no caller-supplied etas / zetas variant: an item that needs its own tables is set up alone afterwards.
 * params: n = gfs_ctx_set_size(s) of them; cfgs: n, or NULL for defaults; item_rc (nullable): n codes, GFS_OK or GFS_NOTHING_TO_DO
 * exactly as the single call returns (an item of 0 nodes; an item with no path of more than one step, which still gets its zeroed
 * position replica).  Returns GFS_OK when every item ended in one of the two ways.
 * Errors: GFS_E_ARG for a null set or params.  Every item's arguments are checked (for _nd: 1..8 dimensions first) before any item
 * is touched and before any device call; the text begins "set item <i>: " and names the lowest failing item; so does a launch
 * shape the policy refuses, found before any item is touched as well.  A device failure after that leaves EVERY item not set up,
 * the arena released, nothing leaked.
 * Ownership: the arena is the set's; the items borrow from it.  A second set setup drops the items' borrows, then reuses or regrows
 * the arena.  gfs_ctx_setup_* on one item afterwards gives that item arrays of its own, the others stay in the arena;
 * gfs_ctx_bind_positions works as before.  gfs_ctx_set_destroy frees the arena after the items.  A gfs_batch made from the items
 * BEFORE a second set setup reads every item's pointers anew at each gfs_batch_run, so it runs from the new arrays — or, where the
 * new launch shape no longer fits it, is refused by its "set up again since the batch was created" check; it never reads freed
 * memory. */
typedef struct gfs_ctx_set_setup_info {
    uint64_t items, configured, nothing_to_do;   /* how the items ended: GFS_OK / GFS_NOTHING_TO_DO */
    uint64_t total_streams, state_bytes;         /* over all items; the one state arena (the seeding tables behind it included) */
    uint64_t device_allocations, copies, launches; /* of this call, counted as gfs_ctx_set_info counts them: hipMalloc + hipHostMalloc
                                                    calls (0 once the arena and the staging have grown), hipMemcpys, kernel launches
                                                    and hipMemsets */
    double   setup_ms;                           /* wall time inside the call */
} gfs_ctx_set_setup_info;

/* The state arrays of a set-up context, in the order they lie in a set's state arena. */
#define GFS_STATE_POSITIONS    0u   /* x_len f64, device order                       */
#define GFS_STATE_COUNTERS     1u   /* 1024 lines of 8 u64                           */
#define GFS_STATE_LEAD         2u   /* team kernels: [8][n_streams] u32              */
#define GFS_STATE_TRACE        3u   /* n_streams * trace_per_stream gfs_term         */
#define GFS_STATE_TRACE_COUNTS 4u   /* n_streams u32                                 */
#define GFS_STATE_RNG          5u   /* [4][n_streams] u64: word k of stream t at k * n_streams + t */
#define GFS_STATE_ZETAS        6u   /* zlen_full f64                                 */
#define GFS_STATE_SCHEDULE     7u   /* iter_max + 1 records of 48 B (IterConsts)     */
#define GFS_STATE_KINDS        8
#define GFS_STATE_SIZE_OF  0x100u   /* or-ed into `which`: the array's size in bytes, as one uint64_t */

/* host only, no device: where item i's state arrays lie in the arena — offsets[8 * i + k] for an array of bytes[8 * i + k] bytes,
 * k = GFS_STATE_*; by kind, then by item; every array starts 256-byte aligned, arrays of a kind are adjacent, none overlap, an
 * array of 0 bytes takes no room; *arena_bytes is the end of the last array's room. */
int      gfs_ctx_set_state_plan(const uint64_t *bytes /*[8*n]*/, uint64_t n, uint64_t *offsets /*[8*n]*/, uint64_t *arena_bytes);
int      gfs_ctx_set_setup_1d(gfs_ctx_set *s, const gfs_sgd_params *params /*[n]*/,
                              const gfs_launch_config *cfgs /*[n], NULL = defaults*/, int32_t *item_rc /*[n], nullable*/);
int      gfs_ctx_set_setup_nd(gfs_ctx_set *s, const gfs_layout_params *params /*[n]*/,
                              const gfs_launch_config *cfgs /*[n], NULL = defaults*/, int32_t *item_rc /*[n], nullable*/);
int      gfs_ctx_set_get_setup_info(const gfs_ctx_set *s, gfs_ctx_set_setup_info *out);   /* of the last set setup; zeros before */
/* test hook, in the style of gfs_ctx_debug_step_records: state array `which` (GFS_STATE_*) of a set-up context — a set's item or
 * not — as it lies on the device; bytes must equal the array's size (0 for an array the setup did not make: nothing is written).
 * which | GFS_STATE_SIZE_OF: that size instead, into a uint64_t (bytes must be 8).  Synchronises. */
int      gfs_ctx_debug_sgd_state(gfs_ctx *ctx, uint32_t which, void *out, uint64_t bytes);

/* ---- multi-device runs (no reference equivalent: the reference is one process, src/sgd.rs:413-593) ----
 * Paths are sharded over `world` ranks, one rank per GPU (one process per GPU, or one host thread per GPU); every rank
 * performs its share of an iteration's term updates on its own replica of the positions; after every window of
 * iterations the replicas are merged.  The collective itself is the CALLER's (RCCL over xGMI: torch.distributed, or
 * ncclAllReduce from the Rust host): the library hands out the device buffer to sum over the ranks and runs the kernels
 * on either side of it.  Only the slots that more than one rank's paths can move are exchanged (all ranks store the
 * positions in one node layout, the default layout's rule applied to the whole graph; a rank's paths touch one span of it);
 * gfs_rank_finish_* completes every replica at the end with one full-length f64 sum.                                  */
#define GFS_MAX_WORLD 64

typedef struct gfs_rank gfs_rank;

typedef struct gfs_rank_config {
    uint32_t rank, world;
    int32_t  device;                  /* HIP device of this rank                                                  */
    uint32_t sharding;                /* 0 auto, 1 consecutive blocks of paths, 2 longest-first bin packing       */
    uint32_t merge_every;             /* iterations per merge window (0 = 1); the last iteration always merges    */
    uint32_t merge_rule;              /* how a window's moves of a slot are merged over the c ranks that moved it:
                                         0 (default): summed move / max(1, c * min(1, window length * eta / mean node length)) —
                                         the mean of the ranks' proposals while the learning rate makes every term a full
                                         correction, their sum once the moves are small steps (multi.hip gfs_rank_window_end);
                                         1 sum; 2 mean over all ranks; 3 summed move / c at every learning rate            */
    uint32_t payload;                 /* exchange buffer element type: 0 f32, 1 f64                               */
    uint32_t exchange;                /* 0: only the slots two or more ranks can move; 1: the whole vector        */
    gfs_launch_config launch;         /* per-rank launch shape; term_updates_per_iteration and stream_base are set
                                         by the library (quota of the rank; rank * n_streams)                     */
} gfs_rank_config;

typedef struct gfs_rank_info {
    uint64_t quota;                   /* this rank's term updates per iteration                                   */
    uint64_t shard_steps;             /* steps of its multi-step paths                                            */
    uint64_t span_lo, span_hi;        /* slots [lo, hi) its paths touch in the shared node layout                 */
    uint64_t shared_slots;            /* slots two or more ranks can move (what a window exchanges)               */
    uint64_t exchange_count;          /* elements of the payload type in the exchange buffer: [delta | touched]   */
    uint64_t positions_len;           /* n_nodes (1D) or n_nodes*2*D                                              */
    uint64_t windows;                 /* merge windows completed                                                  */
    double   last_merge_kernels_ms;   /* prepare + apply kernels of the last window (HIP events)                  */
    uint32_t idle;                    /* 1: no term updates here (no multi-step path in the shard, or quota 0)    */
    uint32_t _pad;
} gfs_rank_info;

/* host-only planning (no device): also what a caller needs to drive gfs_ctx ranks itself */
int gfs_shard_paths(const gfs_graph_view *g, uint32_t world, uint32_t sharding, uint32_t *path_owner /*[n_paths]*/,
                    uint64_t *rank_steps /*[world]*/);
int gfs_shard_quotas(uint64_t term_updates, const uint64_t *rank_steps, uint32_t world, uint64_t *rank_quota /*[world]*/);
int gfs_shared_node_layout(const gfs_graph_view *g, uint32_t *perm /*[n_nodes]*/);
int gfs_exchange_plan(const gfs_graph_view *g, const uint32_t *perm, const uint32_t *path_owner, uint32_t world,
                      uint64_t *span_lo, uint64_t *span_hi /*[world]*/,
                      uint64_t *seg_lo, uint64_t *seg_hi /*[2*world]*/, uint32_t *n_seg,
                      uint64_t *own_lo, uint64_t *own_hi, uint32_t *own_rank /*[2*world+2] or NULL*/, uint32_t *n_own);
/* (own_*: every slot has exactly one designated owner — the lowest rank whose span covers it, rank 0 for slots no span covers —
 * so the intervals tile [0, n_nodes) and gfs_rank_finish_* leaves untouched nodes at their start positions, as sgd.rs:286-294 does) */

/* one rank.  g is the WHOLE graph (every rank derives the same plan from it and keeps only its shard on the device);
 * dims = 0: path_linear_sgd, else path_linear_sgd_layout with that many dimensions.                                  */
int      gfs_rank_create(const gfs_graph_view *g, const gfs_sgd_params *p, uint64_t dims, const gfs_rank_config *cfg,
                         gfs_rank **out);
void     gfs_rank_destroy(gfs_rank *r);
gfs_ctx *gfs_rank_ctx(gfs_rank *r);                               /* the rank's context (stats, raw device pointer)  */
int      gfs_rank_get_info(const gfs_rank *r, gfs_rank_info *out);
int      gfs_rank_set_positions(gfs_rank *r, const double *host, uint64_t n);  /* ABI order; NULL = the reference's 1D start */
int      gfs_rank_positions_changed(gfs_rank *r, void *hip_stream);            /* after writing the device buffer directly */
int      gfs_rank_get_positions(gfs_rank *r, double *host, uint64_t n);        /* complete after gfs_rank_finish_*    */
uint64_t gfs_rank_exchange_count(const gfs_rank *r);
void    *gfs_rank_exchange_buffer(gfs_rank *r);                   /* device pointer (allocated on first use)         */
int      gfs_rank_bind_exchange_buffer(gfs_rank *r, void *device_ptr);         /* use the caller's (a torch tensor)   */
/* a merge window: [this rank's share of iterations ks[0..n), moves -> buffer] | caller: all-reduce(sum) | [apply]    */
int      gfs_rank_window_begin(gfs_rank *r, const uint64_t *ks, uint64_t n, void *hip_stream);
int      gfs_rank_window_end(gfs_rank *r, void *hip_stream);
/* completion: [owned slots -> full (NULL: library scratch, gfs_rank_finish_buffer)] | all-reduce(sum, f64,
 * positions_len) | [full -> positions]                                                                               */
int      gfs_rank_finish_begin(gfs_rank *r, double *full_device, void *hip_stream);
double  *gfs_rank_finish_buffer(gfs_rank *r);
int      gfs_rank_finish_end(gfs_rank *r, const double *full_device, void *hip_stream);
/* the whole schedule.  allreduce must sum device_buf[0..count) over all ranks in place, ordered on hip_stream, and
 * return 0.  Never called when world == 1.                                                                           */
typedef int (*gfs_allreduce_fn)(void *user, void *device_buf, uint64_t count, int is_f64, void *hip_stream);
int      gfs_rank_run(gfs_rank *r, gfs_allreduce_fn allreduce, void *user, void *hip_stream);

/* ---- round-1 whole-vector merge kernels (device pointers), kept for callers that drive gfs_ctx ranks themselves ----
 *   gfs_merge_prepare: buf[0..n) = (float)(x - x_prev), buf[n..2n) = (delta != 0)
 *   all-reduce(sum) of buf over the ranks
 *   gfs_merge_apply  : x_prev += sum_delta / max(1, sum_touched)  (divide_all_by = 0), or
 *                      x_prev += sum_delta / divide_all_by         (1 = plain sum, R = mean); x = x_prev */
int gfs_merge_prepare(const double *x, const double *x_prev, float *buf2n, uint64_t n, void *hip_stream);
int gfs_merge_apply(double *x, double *x_prev, const float *buf2n, uint64_t n, double divide_all_by, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
