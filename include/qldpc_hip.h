/*
 * qldpc_hip.h — C ABI of the MI355X (gfx950) Monte Carlo BP decoding engine.
 *
 * The reference's hot path is Python calling the third-party `ldpc`
 * bp_decoder once per shot.  Each entry point below replaces
 * one reference interface; the Python host layer (qldpc_fault_tolerance_amd/)
 * binds them with ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions: every function returns 0 on success or a negative error code
 * (see QLDPC_E*), and qldpc_last_error() returns a thread-local message.
 * Device pointers (d_*) are plain device addresses (e.g. torch
 * Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = the
 * legacy default stream).  Handles are not thread-safe: one host thread per
 * handle; distinct handles may be used concurrently.
 */
#ifndef QLDPC_HIP_H
#define QLDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLDPC_ABI_VERSION 1

#define QLDPC_OK 0
#define QLDPC_EINVAL -1   /* bad argument (shape, range, NULL)            */
#define QLDPC_EHIP -2     /* HIP runtime error (message has hipGetErrorString) */
#define QLDPC_ENOMEM -3   /* allocation failed                            */
#define QLDPC_ENOTSUP -4  /* graph/method combination not supported       */

/* bp_method, as the strings the reference passes (src/Decoders.py:80-84) */
#define QLDPC_PRODUCT_SUM 0
#define QLDPC_MIN_SUM 1

/* logical_mode = eval_logical_type of CodeSimulator_DataError (src/Simulators.py:162-168) */
#define QLDPC_LOGICAL_X 0
#define QLDPC_LOGICAL_Z 1
#define QLDPC_LOGICAL_TOTAL 2

#define QLDPC_HIST_BINS 1025 /* iteration histogram bins (iter 0..1024; last bin = >=1024) */

typedef struct qldpc_graph qldpc_graph;
typedef struct qldpc_bp qldpc_bp;
typedef struct qldpc_mc qldpc_mc;
typedef struct qldpc_phenl qldpc_phenl;

/* Counters of one fused Monte Carlo run (summed over calls if not reset). */
typedef struct {
  int64_t shots;               /* shots simulated                                */
  int64_t failures;            /* shots whose eval_logical_type outcome failed   */
  int64_t sector_decodes[2];   /* [0] = X errors on hz, [1] = Z errors on hx      */
  int64_t sector_iters[2];     /* sum of BP iterations                            */
  int64_t sector_nonconv[2];   /* decodes that hit max_iter without H x == s      */
  int64_t sector_fail[2];      /* sector failures (syndrome mismatch or logical)  */
  int64_t iter_hist[2][QLDPC_HIST_BINS];
} qldpc_counters;

int qldpc_abi_version(void);
const char *qldpc_last_error(void);
int qldpc_device_count(int *out);

/* Build flags of this library: 0.  QLDPC_BUILD_EXPERIMENTAL is a reserved bit: no build sets it. */
#define QLDPC_BUILD_EXPERIMENTAL 1
int qldpc_build_flags(void);

/*
 * Tanner graph of a parity-check matrix H (m x n), CSR with columns ascending
 * inside each row (the `mod2sparse` order `ldpc` builds from the ndarray it is
 * given: src/Decoders.py:80, `bp_decoder(parity_check_matrix=h, ...)`).
 * Copied to the device; the caller's arrays may be freed after the call.
 */
int qldpc_graph_create(int device, int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                       qldpc_graph **out);
int qldpc_graph_destroy(qldpc_graph *g);
int qldpc_graph_info(const qldpc_graph *g, int32_t *m, int32_t *n, int32_t *nnz, int32_t *max_row_deg,
                     int32_t *max_col_deg);

/*
 * BP decoder on a graph: replaces `ldpc.bp_decoder(parity_check_matrix=h,
 * channel_probs=..., max_iter=..., bp_method=..., ms_scaling_factor=...)`
 * (src/Decoders.py:80-84, :52-56; src/Decoders_SpaceTime.py:207-213).
 *   channel_probs : host array of n doubles (priors log((1-p)/p) computed on
 *                   the host with libm, as the Cython does);
 *   max_iter      : <= 0 means n (ldpc's default);
 *   ms_scaling_factor : alpha; 0 selects alpha = 1 - 2^-iter;
 *   precision     : 64 = float64 messages (reference arithmetic, bit-exact
 *                   with the oracle), 32 = float32 fast mode (same op order).
 *   vars_per_thread : 0 = automatic; else variables per thread (tuning knob).
 *   min_col_slots : 0 = automatic; else edge slots per variable are at least
 *                   this (4 or 8) — lets the two sectors of one MC run share a
 *                   kernel variant when hx and hz have different column degrees.
 */
int qldpc_bp_create(qldpc_graph *g, const double *channel_probs, int32_t max_iter, int32_t bp_method,
                    double ms_scaling_factor, int32_t precision, int32_t vars_per_thread, int32_t min_col_slots,
                    qldpc_bp **out);
int qldpc_bp_destroy(qldpc_bp *bp);
int qldpc_bp_set_channel_probs(qldpc_bp *bp, const double *channel_probs);

/*
 * Decode B syndromes: the batched form of `bp_decoder.decode(synd)` (and
 * BPDecoder.decode, src/Decoders.py:88-90).
 *   d_synd  : uint8 [B][m] 0/1          d_corr : uint8 [B][n] 0/1 (output)
 *   d_iters : int32 [B] or NULL         d_conv : uint8 [B] or NULL
 */
int qldpc_bp_decode_batch(qldpc_bp *bp, const uint8_t *d_synd, uint8_t *d_corr, int32_t *d_iters,
                          uint8_t *d_conv, int64_t B, void *stream);

/*
 * Soft-output BP for BP+OSD (src/Decoders.py:26-41: `bposd_decoder` runs
 * ldpc's BP, then OSD on its final `log_prob_ratios` when BP did not converge).
 * qldpc_bp_create_soft builds a min-sum decoder on engine 1 (the kernel that
 * can write posteriors); qldpc_bp_decode_batch_soft is qldpc_bp_decode_batch
 * plus d_post: double [B][n] = the last iteration's posterior log-probability
 * ratios (ldpc's log_prob_ratios; exact fp32 values widened in fp32 mode).
 * A product-sum decoder (qldpc_bp_create with bp_method 0, engine 5) takes
 * qldpc_bp_decode_batch_soft too: d_post = ldpc bp_decode_prob_ratios'
 * log_prob_ratios = log(1 / posterior ratio) in double (the device's log: equal
 * to libm's except for rare 1-ulp differences).
 */
int qldpc_bp_create_soft(qldpc_graph *g, const double *channel_probs, int32_t max_iter, double ms_scaling_factor,
                         int32_t precision, qldpc_bp **out);
int qldpc_bp_decode_batch_soft(qldpc_bp *bp, const uint8_t *d_synd, uint8_t *d_corr, int32_t *d_iters,
                               uint8_t *d_conv, double *d_post, int64_t B, void *stream);

/*
 * Ordered-statistics decoding (the OSD half of `bposd_decoder(h,
 * channel_probs, max_iter, bp_method, ms_scaling_factor, osd_method,
 * osd_order)`, src/Decoders.py:29-36; BPOSD_Decoder.decode returns
 * `osdw_decoding`, :39-41).  Host-side stage (GF(2) elimination per
 * non-converged syndrome, std::thread pool); all pointers are HOST pointers.
 *   osd_method : 0 = "osd_0", 1 = "osd_e" (exhaustive over 2^osd_order
 *                inputs; the reference's choice), 2 = "osd_cs";
 *   decode     : synd uint8 [B][m], post double [B][n] (BP posteriors), conv
 *                uint8 [B] or NULL (converged shots copy bp_corr [B][n]),
 *                out_osd0 (or NULL) / out_osdw uint8 [B][n];
 *   threads    : <= 0 = OMP_NUM_THREADS if set, else all hardware threads.
 * osd_e takes osd_order <= 20 (a candidate table of 2^order rows).  A syndrome outside the column
 * space of H is solved on the elimination's pivot rows alone, as ldpc's LU solve does.
 */
typedef struct qldpc_osd qldpc_osd;
int qldpc_osd_create(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                     const double *channel_probs, int32_t osd_method, int32_t osd_order, qldpc_osd **out);
int qldpc_osd_destroy(qldpc_osd *osd);
int qldpc_osd_rank(const qldpc_osd *osd, int32_t *rank);
int qldpc_osd_decode_batch(const qldpc_osd *osd, const uint8_t *synd, const double *post, const uint8_t *conv,
                           const uint8_t *bp_corr, uint8_t *out_osd0, uint8_t *out_osdw, int64_t B,
                           int32_t threads);

/*
 * GPU OSD (n <= 8192, osd_e order <= 20 as the host stage): the same outputs as qldpc_osd_decode_batch, one
 * workgroup per syndrome; all pointers are DEVICE pointers (d_post from
 * qldpc_bp_decode_batch_soft).  Uniform channel_probs weigh candidates by popcount; non-uniform
 * ones (the circuit-level DEM priors) by sum log(1/p_j), added in ascending column order as the
 * host stage does.
 */
typedef struct qldpc_osd_gpu qldpc_osd_gpu;
int qldpc_osd_gpu_create(const qldpc_graph *g, const double *channel_probs, int32_t osd_method, int32_t osd_order,
                         qldpc_osd_gpu **out);
int qldpc_osd_gpu_destroy(qldpc_osd_gpu *osd);
int qldpc_osd_gpu_decode(qldpc_osd_gpu *osd, const uint8_t *d_synd, const double *d_post, const uint8_t *d_conv,
                         const uint8_t *d_bp_corr, uint8_t *d_out0, uint8_t *d_outw, int64_t B, void *stream);
/*
 * FirstMinBPDecoder (src/Decoders.py:49-74) on the device: one-iteration min-sum BP (ldpc
 * bp_decoder, max_iter = 1, bp_method "minimum_sum") repeated on the running syndrome while the
 * residual syndrome weight does not grow, at most max_iter accepted steps; the corrections are the
 * xor of the accepted steps' decisions.  One workgroup per syndrome, the whole loop on the device.
 *   create : graph g, channel_probs [n] in (0, 1), max_iter, ms_scaling_factor (0 = ldpc's
 *            1 - 2^-iter schedule at iter 1), precision 64 (ldpc's double) or 32.  QLDPC_ENOTSUP
 *            when 2 (m + n) bytes of arrays and the workgroup kernel's own 16 bytes of LDS exceed
 *            64 KiB, i.e. for m + n > 32760.
 *   decode : device pointers d_synd [B][m] u8 -> d_corr [B][n] u8, d_steps [B] i32 (accepted
 *            steps, or NULL), on `stream`.
 *   info   : the launch qldpc_firstmin_decode would make under the current environment (no
 *            reference counterpart; tests): grid = resident workgroups of the workgroup kernel
 *            (the wave kernel launches up to 4 grid workgroups of 4 waves), lds_bytes = LDS per
 *            workgroup of the kernel it takes, wave = 1 for one wave per syndrome (m + n <= 8192
 *            unless QLDPC_FM_WAVE=0), 0 for one workgroup per syndrome.  Any output may be NULL.
 * Replaces the Python loop of FirstMinBPDecoder.decode (Decoders.py:60-74).
 */
typedef struct qldpc_firstmin qldpc_firstmin;
/* qldpc_phenl_set_round_firstmin (declared after qldpc_phenl below) makes the noisy rounds of the
 * phenomenological pipeline decode with these (CodeSimulator_Phenon with FirstMinBPDecoder decoder1,
 * the Single-Shot notebook's configuration). */
int qldpc_firstmin_create(const qldpc_graph *g, const double *channel_probs, int32_t max_iter,
                          double ms_scaling_factor, int32_t precision, qldpc_firstmin **out);
int qldpc_firstmin_destroy(qldpc_firstmin *fm);
int qldpc_firstmin_info(const qldpc_firstmin *fm, int32_t *grid, int32_t *lds_bytes, int32_t *wave);
int qldpc_firstmin_decode(qldpc_firstmin *fm, const uint8_t *d_synd, uint8_t *d_corr, int32_t *d_steps, int64_t B,
                          void *stream);

/* Elimination geometry the handle chose (no reference counterpart; tests and DESIGN.md §4):
 * row_words = 64-bit words per register row (0: LDS / HBM image), window_words = always 0 (no
 * layout holds a column window; the argument stays for the ABI), threads = per workgroup,
 * workgroups = the launch's persistent grid. */
int qldpc_osd_gpu_geometry(const qldpc_osd_gpu *osd, int32_t *row_words, int32_t *window_words, int32_t *threads,
                           int32_t *workgroups);

/*
 * BP+LSD: localised statistics decoding of order 0 (Hillmann et al. 2024; ldpc v2's BpLsdDecoder) as the
 * second stage in place of OSD, through the same two handles (csrc/lsd.hip).
 * THE LAW.  Inputs for one syndrome: H (m x n), the syndrome s, the posteriors L[n] (double: BP's
 * log_prob_ratios, what the OSD stage receives) and bits_per_step = k >= 1.  Every choice below is a set
 * or a total order, so no execution order can change a result.
 *   column order : j comes before j' when L_j < L_j' as doubles, or when neither is less and j < j' (the
 *                  OSD stage's stable ascending sort: -0 and +0 tie, +-inf are ordered, NaN is unspecified).
 *   state        : active columns A (empty at first), active rows R (at first {i : s_i = 1}); every row
 *                  adjacent to a column of A is in R.
 *   clusters     : the connected components of the bipartite graph on R and A with the edges of H; a seed
 *                  row without an active column is a cluster of its own.  A cluster C is valid when s on
 *                  its rows lies in the column space of H[rows(C), cols(C)].
 *   round        : every invalid cluster nominates the first min(k, |boundary|) columns of its boundary
 *                  (the columns outside A adjacent to one of its rows) in column order; all nominated
 *                  columns join A at once (a column nominated twice joins once) and their rows join R;
 *                  clusters and validity are formed anew (a merge can make a valid cluster invalid again,
 *                  and the reverse).  Rounds repeat until no invalid cluster has a boundary column; an
 *                  invalid cluster without boundary is unsolvable (it holds its whole component of the
 *                  Tanner graph and is still inconsistent).
 *   output       : x_j = 0 outside A and on the columns of unsolvable clusters; on each valid cluster x is
 *                  its OSD-0 solution: walk its columns in column order, keep each column independent of
 *                  the kept ones, x = the unique solution supported on the kept columns.
 *   statistics   : int32 [4] = valid (1: no unsolvable cluster), rounds (those that added a column), |A|,
 *                  clusters at the end.  An all-zero syndrome gives x = 0 and (1, 0, 0, 0), as a
 *                  converged entry does (which copies bp_corr).
 * The stage uses no channel weights: order 0 weighs no candidates.
 * qldpc_osd_create_lsd: a host stage.  qldpc_osd_decode_batch on it writes the law's x to out_osd0 (if
 * given) and out_osdw; qldpc_osd_set_side_probs succeeds and a side decode equals the plain decode;
 * qldpc_osd_rank answers.  QLDPC_EINVAL: bits_per_step < 1, NULL, a bad shape or column index.
 * qldpc_lsd_decode_batch_stats: the same decode plus stats int32 [B][4] (or NULL); LSD handles only.
 * qldpc_osd_gpu_create_lsd: the GPU stage, m, n <= 8192 (QLDPC_ENOTSUP past it), one 256-thread
 * workgroup per non-converged syndrome.  Every qldpc_osd_gpu_decode* call, qldpc_mc_set_osd,
 * qldpc_mc_set_staged_osd, qldpc_phenl_set_final_osd and qldpc_circ_set_final_osd take such a handle
 * (the latter also a host LSD stage); qldpc_osd_gpu_geometry answers row_words = 0 and the launch.
 * qldpc_lsd_gpu_decode adds d_stats int32 [B][4] (or NULL) and writes one output.  The active image
 * lives in LDS up to a row capacity cut at create time (qldpc_lsd_gpu_info: lds_rows, 0 = none, and the
 * LDS bytes per workgroup); a syndrome that outgrows it, or every syndrome under QLDPC_LSD_WS=1, is
 * decoded on the workgroup's HBM slice, with the same answer.
 */
int qldpc_osd_create_lsd(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                         int32_t bits_per_step, qldpc_osd **out);
int qldpc_lsd_decode_batch_stats(const qldpc_osd *osd, const uint8_t *synd, const double *post, const uint8_t *conv,
                                 const uint8_t *bp_corr, uint8_t *out, int32_t *stats, int64_t B, int32_t threads);
int qldpc_osd_gpu_create_lsd(const qldpc_graph *g, int32_t bits_per_step, qldpc_osd_gpu **out);
int qldpc_lsd_gpu_decode(qldpc_osd_gpu *osd, const uint8_t *d_synd, const double *d_post, const uint8_t *d_conv,
                         const uint8_t *d_bp_corr, uint8_t *d_out, int32_t *d_stats, int64_t B, void *stream);
int qldpc_lsd_gpu_info(const qldpc_osd_gpu *osd, int32_t *lds_rows, int32_t *lds_bytes);
/* decodes since the last call that outgrew the LDS image and ran again on the HBM slice; waits for the device */
int qldpc_lsd_gpu_retries(qldpc_osd_gpu *osd, uint64_t *count);

/*
 * BP+LSD of higher order (ldpc v2's lsd_order / lsd_method): the clusters grow until each has a few dependent
 * ("free") columns, and a handful of candidates per cluster is weighed by channel weight.
 * THE LAW.  Inputs: everything the order-0 law above takes, lsd_method in {0 = "lsd_0", 1 = "lsd_e",
 * 2 = "lsd_cs"}, lsd_order = w >= 0 and priors p_j in (0, 1).  Order 0, or method 0, is the order-0 law bit
 * for bit.  Every choice is again a set or a total order.
 *   weights    : wq_j = floor(log(1 / p_j) 2^32 + 0.5) as a 64-bit integer, computed once on the host with
 *                std::log (as Relay-BP's wq).  A candidate weighs the sum of wq_j over x_j = 1: an integer
 *                sum, so any summation order is allowed; uniform priors give popcount order.
 *   free count : free(C) = |cols(C)| - rank(H[rows(C), cols(C)]).
 *   round      : a cluster nominates the first min(k, |boundary|) boundary columns in column order when it is
 *                invalid, or when it is valid and free(C) < w.  Everything else in a round is unchanged (all
 *                nominated columns join at once, clusters and validity are formed anew, a merge may
 *                invalidate a cluster).  Rounds end when no nominating cluster has a boundary column.
 *   split      : on each valid final cluster, walk its columns in column order as OSD-0 does: the kept columns
 *                P (the pivots) and the free columns F, in column order; each free column f equals a unique
 *                xor dep(f) of earlier kept columns.
 *   candidates : candidate 0 is the OSD-0 solution x0.  Later candidates are sets t of free columns with
 *                x(t) = x0 + sum over f in t of (e_f + dep(f)) (mod 2).  T = the first min(w, |F|) columns
 *                of F.  lsd_e: all non-empty subsets of T in natural binary order, bit i for T[i].  lsd_cs:
 *                {f} for every f in F in column order, then {T[a], T[b]} for a < b in lexicographic order.
 *                The first strictly lighter candidate wins, cluster by cluster.  Unsolvable clusters and
 *                everything outside A stay 0.
 *   outputs    : out_osd0 = the union of the candidates 0 on the grown clusters; out_osdw = the union of the
 *                winners.  Statistics as above (growth rounds count).
 * lsd_e takes w <= 12, lsd_cs w <= 64.  QLDPC_EINVAL: an order past those, a negative order, an unknown method,
 * and with an order above 0 in force a prior outside (0, 1) or no priors.
 * qldpc_osd_create_lsd_order / qldpc_osd_gpu_create_lsd_order: the handles of qldpc_osd_create_lsd /
 * qldpc_osd_gpu_create_lsd (which mean order 0), served by the same calls.  channel_probs may be NULL at
 * order 0.  With an order above 0 in force there are no per-shot side tables: qldpc_osd_set_side_probs and
 * qldpc_osd_gpu_set_side_probs return QLDPC_ENOTSUP.  The GPU stage keeps dep(f) of every free column
 * beside the image (as many as rows in LDS; a decode with more is taken again on the HBM slice and counted
 * by qldpc_lsd_gpu_retries) and spreads each cluster's candidates over the workgroup.
 * A GPU handle of order > 0 keeps 4 m more bytes of tables in LDS than one of order 0: where that exceeds the
 * 160 KiB of a workgroup (n = 8192 with m above about 7,500) the create call returns QLDPC_ENOTSUP although
 * the order-0 handle exists.
 * qldpc_lsd_weights: the handle's wq [n] (QLDPC_EINVAL on a stage created without priors in (0, 1)).
 */
int qldpc_osd_create_lsd_order(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                               const double *channel_probs, int32_t bits_per_step, int32_t lsd_method,
                               int32_t lsd_order, qldpc_osd **out);
int qldpc_osd_gpu_create_lsd_order(const qldpc_graph *g, const double *channel_probs, int32_t bits_per_step,
                                   int32_t lsd_method, int32_t lsd_order, qldpc_osd_gpu **out);
int qldpc_lsd_weights(const qldpc_osd *osd, int64_t *wq);

/*
 * Fused Monte Carlo shot loop = CodeSimulator_DataError._single_run
 * (src/Simulators.py:117-168) for many shots in one launch: per shot sample
 * the Pauli error (3-way split of u, :99-113), syndrome H e, BP decode,
 * residual, failure = (H r != 0) or (L r != 0).
 *   dec_x, logical_x : decoder on hz and the lz logicals (sector X);
 *   dec_z, logical_z : decoder on hx and the lx logicals (sector Z); either
 *                      sector may be NULL if logical_mode does not need it.
 * Shots are keyed by their global index: shot s, qubit j draws
 * u = Philox4x32-10(key = seed, ctr = (j, s_lo, s_hi, stream)) as a 53-bit
 * double, so any shot range sharded over devices reproduces the same counts.
 * The sectors need not match: hx and hz may differ in rows and degrees, and their decoders in
 * engine, threads, vars per thread, degree class, precision or layout family.  One fused kernel
 * serves a pair whose routes agree (row counts, row widths and degree-3 slot counts may differ);
 * any other pair runs the staged pipeline (qldpc_mc_create_staged), bit-identical per shot.
 * Different code lengths or devices are QLDPC_EINVAL.
 */
int qldpc_mc_create(qldpc_bp *dec_x, const qldpc_graph *logical_x, qldpc_bp *dec_z,
                    const qldpc_graph *logical_z, qldpc_mc **out);
int qldpc_mc_destroy(qldpc_mc *mc);

/* Async launch: counters accumulate in device memory (d_counters, a
 * qldpc_counters-sized device buffer, zeroed by the caller).  uniforms: NULL
 * => Philox, else device doubles [shot_count][n] (bit-exact replays of an
 * external u stream, e.g. CPython random()).  Optional per-shot outputs
 * (device, NULL to skip): d_fail uint8 [S] (bit0 X-sector fail, bit1 Z),
 * d_err uint8 [S][n] (bit0 x, bit1 z), d_corr uint8 [S][2][n], d_iters
 * int32 [S][2].  grid_blocks <= 0 selects a persistent grid sized to the device.
 */
int qldpc_mc_launch(qldpc_mc *mc, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                    int64_t shot_count, int32_t logical_mode, const double *d_uniforms, void *d_counters,
                    uint8_t *d_fail, uint8_t *d_err, uint8_t *d_corr, int32_t *d_iters, int32_t grid_blocks,
                    void *stream);

/*
 * qldpc_mc_create with the staged pipeline forced (sample -> H e -> unpack -> qldpc_bp_decode_batch ->
 * fold -> [H; L] check -> tally, bit-sliced 64 shots per word) whatever the decoders' routes: the
 * handle qldpc_mc_launch_weight needs.  Same arguments and contract as qldpc_mc_create;
 * qldpc_mc_launch / qldpc_mc_run work on it as on any handle; qldpc_mc_set_osd does not.
 */
int qldpc_mc_create_staged(qldpc_bp *dec_x, const qldpc_graph *logical_x, qldpc_bp *dec_z,
                           const qldpc_graph *logical_z, qldpc_mc **out);

/*
 * The shot loop on errors of FIXED weight: every shot's error is a uniform random `weight`-subset of
 * the n qubits with i.i.d. Pauli classes in the ratio px : py : pz (a depolarizing error conditioned
 * on its weight; the decoders keep their own priors).  Shot s, step i = 0 .. weight-1, t = n - weight + i:
 * (o0..o3) = Philox4x32-10(key = seed, ctr = (i, s_lo, s_hi, 0x51D50006)); r = (((o1 << 32) | o0) *
 * (t + 1)) >> 64; the step takes qubit r, or qubit t if r is taken already (Floyd's algorithm); its
 * class is Z if k < ceil(2^53 pz / T), else X if k < ceil(2^53 (pz + px) / T), else Y, with
 * k = ((o2 >> 5) << 26) | (o3 >> 6) and T = (pz + px) + py.  A shot depends on (seed, s, weight, n,
 * px : py : pz) only; the same (seed, s) at two weights shares draws, so give every weight its own
 * shot range.  Counters and optional per-shot outputs as qldpc_mc_launch.  Needs a handle of
 * qldpc_mc_create_staged (or any staged handle) without OSD: QLDPC_ENOTSUP otherwise, and for
 * n > 4096.  QLDPC_EINVAL: weight outside 0 .. n, a negative probability, px = py = pz = 0 with
 * weight > 0.
 */
int qldpc_mc_launch_weight(qldpc_mc *mc, int32_t weight, double px, double py, double pz, uint64_t seed,
                           uint64_t shot_begin, int64_t shot_count, int32_t logical_mode, void *d_counters,
                           uint8_t *d_fail, uint8_t *d_err, uint8_t *d_corr, int32_t *d_iters, void *stream);

/* Synchronous convenience: launch + copy counters to host (accumulating into *out). */
int qldpc_mc_run(qldpc_mc *mc, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                 int64_t shot_count, int32_t logical_mode, qldpc_counters *out, void *stream);

/*
 * Phenomenological space-time shot loop = CodeSimulator_Phenon_SpaceTime
 * (src/Simulators_SpaceTime.py:382-548): per sample, num_rounds - 1 noisy
 * rounds of num_rep repetitions (fresh depolarizing data error + syndrome
 * flips with probability q, :395-431), each decoded by BP on the stacked
 * space-time graph (ST_BP_Decoder_syndrome, src/Decoders_SpaceTime.py:200-223)
 * from its detector history (Z sector differenced, X sector raw: quirk Q3,
 * :464-476), then a perfect final round decoded by dec2 and the failure check
 * of :500-529.
 *   st_x / st_z   : decoders on GetSpaceTimeCheckMat(hz / hx, num_rep)
 *                   (checked against the final decoders' graphs);
 *   dec2_x/dec2_z : final-round decoders on hz / hx;
 *   logical_x/_z  : lz / lx.
 *   max_batch     : samples in flight per pass (0 = 65536); device buffers
 *                   are sized for it at create time.
 * Both sectors are required (the uniform stream interleaves both check sets).
 */
int qldpc_phenl_create(qldpc_bp *st_x, qldpc_bp *st_z, qldpc_bp *dec2_x, qldpc_bp *dec2_z,
                       const qldpc_graph *logical_x, const qldpc_graph *logical_z, int32_t num_rep, int64_t max_batch,
                       qldpc_phenl **out);
int qldpc_phenl_destroy(qldpc_phenl *ph);
/* Bytes per sample of the optional trace: per noisy round the Z then X
 * detector histories ([num_rep][m_x], [num_rep][m_z]), then the final Z and X
 * syndromes. */
int qldpc_phenl_trace_len(const qldpc_phenl *ph, int32_t num_rounds, int64_t *out);
/* Async launch on `stream`; counters accumulate into d_counters (device
 * qldpc_counters, zeroed by the caller; sector_* count the ST and final
 * decodes).  Sample s uses global index shot_begin + s for its Philox stream,
 * or d_uniforms[s][n_u] (n_u = ((num_rounds-1)*num_rep + 1)*(n + m_x + m_z),
 * CPython's draw order) when non-NULL.  d_fail uint8 [S] (bit0 X, bit1 Z) and
 * d_trace uint8 [S][trace_len] are optional. */
int qldpc_phenl_launch(qldpc_phenl *ph, double px, double py, double pz, double q, uint64_t seed,
                       uint64_t shot_begin, int64_t shot_count, int32_t num_rounds, int32_t logical_mode,
                       const double *d_uniforms, void *d_counters, uint8_t *d_fail, uint8_t *d_trace, void *stream);

/* BP+OSD as the final-round decoder (decoder2 = BPOSD_Decoder in the
 * notebooks, src/Decoders.py:100-138): the sectors given a GPU OSD handle
 * decode the perfect round with soft BP (dec2 must come from
 * qldpc_bp_create_soft) and then OSD where BP did not converge.  NULL = plain
 * BP for that sector.  Declared after qldpc_osd_gpu above. */
int qldpc_phenl_set_final_osd(qldpc_phenl *ph, qldpc_osd_gpu *osd_x, qldpc_osd_gpu *osd_z);
/* Noisy rounds decoded by FirstMinBPDecoder (qldpc_firstmin_*, built on exactly the ST graph of st_x /
 * st_z) instead of BP; NULL keeps BP for that sector.  The trace counters then hold the accepted
 * first-min steps as iterations and count no non-converged decodes for those rounds. */
int qldpc_phenl_set_round_firstmin(qldpc_phenl *ph, qldpc_firstmin *fm_x, qldpc_firstmin *fm_z);

/* Launch geometry chosen for a decoder (threads per shot, vars per thread,
 * LDS bytes, resident blocks per CU) — reported by bench.py / DESIGN.md. */
int qldpc_bp_geometry(const qldpc_bp *bp, int32_t *threads, int32_t *vars_per_thread, int32_t *lds_bytes,
                      int32_t *blocks_per_cu);

/* Kernel engine serving a decoder: 3 = register-resident variables (default
 * when the graph fits: column degree <= 4, <= 8 variables per thread, image
 * < 64 KiB), 2 = streamed variables, 1 = LDS-atomic check state, 5 = product-sum
 * (bp_method 0), 6 = HBM-resident messages (qldpc_bp_create_hbm; automatic for images over
 * 160 KiB), 7 = Relay-BP (qldpc_bp_create_relay), 8 = serial-schedule min-sum
 * (qldpc_bp_create_serial).  QLDPC_ENGINE in the environment selects 1, 2 or 6 explicitly
 * (4, a removed engine, answers QLDPC_ENOTSUP). */
int qldpc_bp_engine(const qldpc_bp *bp, int32_t *engine);

/* Compile-time family of the decoder's kernels (the ENG template argument of rmc_kernel /
 * rdec_kernel as rocprofv3 prints it): engine 3 = 3, 13 (dword-scaled addresses), 103 (fp64
 * <= 256 threads), 1013 (tail layout, 1024 threads), 11103 (fp64 m2-in-slot, rows of 3 chunks +
 * a tail slot, 3 workgroups per CU); other engines their number.
 * row_chunks = 16-byte chunks per check row (engines 2-3). */
int qldpc_bp_kernel_id(const qldpc_bp *bp, int32_t *kernel_id, int32_t *row_chunks);

/* The route qldpc_bp_create would take for this graph, priors and the QLDPC_* switches, decided
 * on the host alone (no device call: runs on a machine without a GPU).  out[0..7] = engine,
 * kernel_id, row_chunks, threads, vars_per_thread, lds_bytes, degree3_slots, degree2_slots as the
 * decoder's qldpc_bp_engine / _kernel_id / _geometry / _degree3_slots report them; out_len >= 8.
 * The errors of qldpc_bp_create that do not involve the device; ENOTSUP for product-sum. */
int qldpc_bp_plan(const qldpc_graph *g, const double *channel_probs, int32_t bp_method, int32_t precision,
                  int32_t vars_per_thread, int32_t min_col_slots, int32_t *out, int32_t out_len);

/* Engine 3: leading variable slots per thread that hold only variables of
 * column degree <= 3 (variables are host-sorted by degree; those slots skip the
 * 4th edge slot at compile time).  0 for the other engines and for the fp64
 * kernels of workgroups wider than 256 threads. */
int qldpc_bp_degree3_slots(const qldpc_bp *bp, int32_t *d3k);

/* Min-sum decoder on engine 6 (bp_hbm.hip): messages in HBM as coalesced
 * [edge][lane] arrays, one decode per lane, waves independent.  The engine every
 * create call falls back to when no LDS engine holds a decode's image (> 160
 * KiB: e.g. the fp64 space-time graph of hgp_34_n1225_q3 at num_rep 3) or a
 * column degree exceeds 8; this entry point forces it for any graph (row and
 * column degree <= 12: the compile-time edge blocks kHRow / kHCol of bp_hbm.hip;
 * larger degrees return QLDPC_ENOTSUP).  Same decode contract as qldpc_bp_create (the ldpc
 * bp_decoder replacement, src/Decoders.py:80-84); min-sum only. */
int qldpc_bp_create_hbm(qldpc_graph *g, const double *channel_probs, int32_t max_iter, double ms_scaling_factor,
                        int32_t precision, qldpc_bp **out);

/*
 * Relay-BP (Mueller et al. 2025) on engine 7 (relay.hip): min-sum BP with a per-variable memory term,
 * run as a chain of legs that collects up to stop_nconv syndrome-consistent solutions and keeps the
 * lightest.  No reference counterpart: the decoder for the slot after plain BP, with no elimination.
 * THE LAW, T = double (precision 64) or float (32), every operation in T in ldpc's min-sum order:
 *   L0_j = (T) log((1 - p_j) / p_j) (double, libm);  wq_j = (int64) floor(L0_j(double) 2^32 + 0.5);
 *   gam[0][j] = (T) pre_gamma;  gam[r][j] = (T)(gamma_lo + (gamma_hi - gamma_lo) u) in double, r = 1 ..
 *     num_legs, u = ((o0 >> 5) 2^26 + (o1 >> 6)) / 2^53, (o0..o3) = Philox4x32-10(key = (seed_lo, seed_hi),
 *     ctr = (j, r, 0, 0x51D50007));
 *   M_j <- L0_j, nsol <- 0, bestW <- +inf, iters <- 0;  for leg r = 0 .. num_legs (pre_iter iterations
 *   for r = 0, else leg_iter):  bias_j = ((T)1 - gam[r][j]) L0_j + gam[r][j] M_j (two rounded products
 *   and one rounded sum, never an FMA); every bit-to-check message of column j <- bias_j; each iteration
 *   t = 1 .. : ldpc's min-sum check pass (alpha = ms_scaling_factor, or 1 - 2^-t when that is 0), its
 *   variable pass with bias_j (from the current M_j) in place of the prior, M_j <- the column's final
 *   sum, dec_j = (M_j <= 0), iters += 1; the leg ends when H dec == s.  A leg that ended so is a solution:
 *   nsol += 1, W = sum of wq_j over dec_j = 1, best <- dec when W < bestW (strict); the chain stops at
 *   nsol == stop_nconv.  M carries into the next leg; the messages restart from the new bias.
 *   corr = best if nsol > 0 else the last dec; conv = (nsol > 0); iters <= pre_iter + num_legs leg_iter.
 * num_legs = 0 and pre_gamma = 0 is plain min-sum BP, bit for bit.
 *
 * qldpc_bp_create_relay returns an ordinary qldpc_bp (qldpc_bp_engine: 7; max_iter = pre_iter +
 * num_legs leg_iter) for qldpc_bp_decode_batch and every loop that decodes through it: the staged
 * data-error pipeline (qldpc_mc_create sends it there), qldpc_mc_launch_weight, the phenomenological
 * and circuit loops.  qldpc_bp_set_channel_probs rebuilds L0 and the weights.  No soft output
 * (qldpc_bp_decode_batch_soft) and no qldpc_mc_set_osd: QLDPC_ENOTSUP.  One decode per 256-thread
 * workgroup, the whole chain in the kernel; state in LDS when it fits 160 KiB, else the messages in an
 * HBM workspace (QLDPC_RELAY_WS=1 forces that); the graph's index arrays are staged in LDS as 16-bit
 * words when that costs no resident workgroup (QLDPC_RELAY_IDX=0: walked in global memory).  QLDPC_EINVAL: pre_iter < 1, num_legs < 0, leg_iter <
 * 1 with num_legs > 0, stop_nconv < 1, gamma_lo > gamma_hi, a non-finite gamma, precision not 32 / 64.
 * qldpc_relay_gammas: the gamma table alone, host only, widened to double, out [num_legs + 1][n].
 * qldpc_relay_decode_host: the same law in plain C++ on host memory (no HIP call, any graph): synd
 * [B][m], corr [B][n], iters / conv / nsol [B] (each may be NULL); threads <= 0 = OMP_NUM_THREADS if
 * set, else all hardware threads.
 */
int qldpc_bp_create_relay(qldpc_graph *g, const double *channel_probs, int32_t pre_iter, double pre_gamma,
                          int32_t num_legs, int32_t leg_iter, double gamma_lo, double gamma_hi, int32_t stop_nconv,
                          uint64_t gamma_seed, double ms_scaling_factor, int32_t precision, qldpc_bp **out);
int qldpc_relay_gammas(int32_t n, double pre_gamma, int32_t num_legs, double gamma_lo, double gamma_hi,
                       uint64_t gamma_seed, int32_t precision, double *out);
int qldpc_relay_decode_host(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                            const double *channel_probs, int32_t pre_iter, double pre_gamma, int32_t num_legs,
                            int32_t leg_iter, double gamma_lo, double gamma_hi, int32_t stop_nconv,
                            uint64_t gamma_seed, double ms_scaling_factor, int32_t precision, const uint8_t *synd,
                            uint8_t *corr, int32_t *iters, uint8_t *conv, int32_t *nsol, int64_t B, int32_t threads);

/*
 * Min-sum BP on the serial (variable-by-variable, "layered") schedule, engine 8 (serial.hip).  No
 * reference counterpart (the reference's ldpc release offered the flooding schedule only; current ldpc
 * calls this schedule="serial").
 * THE LAW, T = double (precision 64) or float (32), every operation in T, the primitives those of
 * ldpc's min-sum:
 *   priors   L0_j = (T) log((1 - p_j) / p_j), computed in double with libm.
 *   layers   layer(j) is the smallest l >= 0 such that no variable j' < j with layer(j') = l shares a
 *            check with j: first-fit in ascending variable index.  The sweep order pi is the variables
 *            sorted by (layer, index).  Two variables of one layer share no check, so updating a layer in
 *            parallel equals the sequential sweep in order pi.  The host law is that sequential sweep.
 *   start    b2c[e] = L0_col(e) for every edge.
 *   iteration t = 1 .. max_iter: a_t = (T) ms_scaling_factor, or (T)(1 - 2^-t) when ms_scaling_factor
 *            is 0.  For each variable j in order pi:
 *            1. for each edge e of column j, rows ascending, with i = row(e): mag = the minimum of
 *               |b2c[e']| over the other edges e' of row i, or the sentinel (1e308 for double, FLT_MAX
 *               for float) when there is none; s = synd_i + the number of those e' with b2c[e'] <= 0;
 *               c2b[e] = mag * (s odd ? -a_t : a_t);
 *            2. the variable pass of min-sum on column j alone: forward over the column's edges, temp =
 *               L0_j, for each edge b2c[e] = temp, temp = temp + c2b[e]; post_j = temp, dec_j = (temp <=
 *               0); backward, temp = 0, for each edge in reverse b2c[e] = b2c[e] + temp, temp = temp +
 *               c2b[e].
 *            After the sweep iters = t.  The decode stops with conv = 1 when H dec == synd.
 *   output   corr = dec of the last sweep; iters; conv.  The soft output is post_j widened to double,
 *            laid out like qldpc_bp_create_soft's posteriors ([B][n]).
 * A minimum and a parity count do not depend on the order in which a row is walked, so the kernel may
 * read a row in any order; the column sums keep the stated order.
 *
 * qldpc_bp_create_serial returns an ordinary qldpc_bp (qldpc_bp_engine: 8) for qldpc_bp_decode_batch
 * and, with soft = 1, qldpc_bp_decode_batch_soft, and for every loop that decodes through a qldpc_bp:
 * the staged data-error pipeline (qldpc_mc_create sends it there), qldpc_mc_launch_weight, the
 * phenomenological and circuit loops.  qldpc_bp_set_channel_probs rebuilds L0.  No qldpc_mc_set_osd
 * and no qldpc_phenl_set_final_osd: QLDPC_ENOTSUP.  Min-sum only.  QLDPC_EINVAL: max_iter < 1, a
 * precision other than 32 / 64.  One decode per workgroup (64, 128 or 256 threads: the widest layer
 * decides; QLDPC_SERIAL_TB overrides), the whole decode in the kernel; b2c in LDS when the image fits
 * 160 KiB, else in an HBM workspace (QLDPC_SERIAL_WS=1 forces that); the index arrays and the layer
 * table are staged in LDS as 16-bit words when they fit that range and cost no resident workgroup
 * (QLDPC_SERIAL_IDX=0: walked in global memory).
 * qldpc_serial_layers: layer(j) of every variable and the number of layers, host only.
 * qldpc_serial_decode_host: the law in plain C++ on host memory (no HIP call, any graph): synd [B][m],
 * corr [B][n], iters / conv [B], post [B][n] (each of the three may be NULL); threads <= 0 =
 * OMP_NUM_THREADS if set, else all hardware threads.
 */
int qldpc_bp_create_serial(qldpc_graph *g, const double *channel_probs, int32_t max_iter, double ms_scaling_factor,
                           int32_t precision, int32_t soft, qldpc_bp **out);
int qldpc_serial_layers(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, int32_t *layer_out,
                        int32_t *num_layers);
int qldpc_serial_decode_host(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                             const double *channel_probs, int32_t max_iter, double ms_scaling_factor,
                             int32_t precision, const uint8_t *synd, uint8_t *corr, int32_t *iters, uint8_t *conv,
                             double *post, int64_t B, int32_t threads);

/*
 * Side priors: per-syndrome, per-variable priors selected by a byte, for X/Z-correlated decoding (bposd's
 * css_decode_sim(channel_update="x->z" | "z->x")): one sector is decoded first, and the other sector's
 * decoder is given, per shot and qubit, the prior conditioned on the first decoder's decision.
 * THE LAW.  A decoder of engine 7 or 8 may carry two probability tables p0[n], p1[n], every entry
 * finite and strictly inside (0, 1).  A side decode takes, beside the syndromes, d_side: uint8 [B][n],
 * of which only bit 0 is read (0xFE counts as 0, 0x03 as 1).  For syndrome b and variable j,
 *   L0_j = (T) log((1 - q) / q),  q = (side[b][j] & 1) ? p1[j] : p0[j],
 * computed on the host in double with libm and cast to T, exactly as the plain handle's table.  Everything
 * else is the engine's law above with that L0.  Engine 7: M_j <- L0_j; bias_j = ((T)1 - gam) L0_j + gam
 * M_j; the solution weights wq_j = (int64) floor(L0_j(double) 2^32 + 0.5) come from the same selected
 * prior (two integer weight tables).  Engine 8: the start value of b2c, and temp = L0_j in the variable
 * pass.  q = 0.5 gives L0 = +0, and the decision rule temp <= 0 -> 1 stays as it is.  A side decode with
 * side = 0 everywhere and p0 = channel_probs is the plain decode, bit for bit; with side = 1 everywhere it
 * is the plain decode of a handle built on p1.
 *
 * qldpc_bp_set_side_probs: engines 7 and 8 only (QLDPC_ENOTSUP otherwise); QLDPC_EINVAL for an entry
 * outside (0, 1) or non-finite; may be called again to replace the tables; touches neither the handle's
 * ordinary priors nor any other entry point's result, nor qldpc_bp_geometry.
 * qldpc_bp_decode_batch_side: qldpc_bp_decode_batch with d_side; QLDPC_EINVAL when no side tables are
 * set.  No soft output.  The kernels read each side byte once per syndrome and keep its bit in bit 1 of
 * the decision byte the decode already holds in LDS, so a side decode runs on the plain decode's LDS
 * image and workgroup width (qldpc_bp_geometry reports one geometry for both; the persistent grid of a
 * side decode is the side variant's own residency, at most the plain grid), and its variable pass
 * issues the same single global load for the prior, from a two-row table.
 * qldpc_relay_decode_host_side / qldpc_serial_decode_host_side: the law in plain C++ on host memory;
 * the arguments of qldpc_relay_decode_host / qldpc_serial_decode_host with p0, p1, side [B][n] in the
 * place of channel_probs (the serial form without the posteriors).
 */
int qldpc_bp_set_side_probs(qldpc_bp *bp, const double *p0, const double *p1);
int qldpc_bp_decode_batch_side(qldpc_bp *bp, const uint8_t *d_synd, const uint8_t *d_side, uint8_t *d_corr,
                               int32_t *d_iters, uint8_t *d_conv, int64_t B, void *stream);
/* Soft output of a side decode: corr / iters / conv exactly as qldpc_bp_decode_batch_side returns them
 * (d_side = NULL: as qldpc_bp_decode_batch), and d_post [B][n], the posteriors after the last iteration.
 * Engine 8: handles created with soft = 1 (post_j widened to double, as qldpc_bp_decode_batch_soft).
 * Engine 7: handles with num_legs = 0 only; d_post[b][j] = (double) M_j after the last iteration, which
 * with pre_gamma = 0 is ldpc's log_prob_ratios bit for bit.  The kernel writes the M it already holds in
 * LDS in its output loop: no LDS byte, no barrier, one qldpc_bp_geometry.  QLDPC_ENOTSUP: any other
 * engine, an engine-8 handle without soft, an engine-7 chain (num_legs > 0: a chain's best solution has
 * no single posterior).  QLDPC_EINVAL: d_side without side tables.  qldpc_bp_decode_batch_soft keeps
 * refusing engine 7. */
int qldpc_bp_decode_batch_side_soft(qldpc_bp *bp, const uint8_t *d_synd, const uint8_t *d_side, uint8_t *d_corr,
                                    int32_t *d_iters, uint8_t *d_conv, double *d_post, int64_t B, void *stream);
int qldpc_relay_decode_host_side(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                                 const double *p0, const double *p1, const uint8_t *side, int32_t pre_iter,
                                 double pre_gamma, int32_t num_legs, int32_t leg_iter, double gamma_lo,
                                 double gamma_hi, int32_t stop_nconv, uint64_t gamma_seed, double ms_scaling_factor,
                                 int32_t precision, const uint8_t *synd, uint8_t *corr, int32_t *iters, uint8_t *conv,
                                 int32_t *nsol, int64_t B, int32_t threads);
int qldpc_serial_decode_host_side(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx,
                                  const double *p0, const double *p1, const uint8_t *side, int32_t max_iter,
                                  double ms_scaling_factor, int32_t precision, const uint8_t *synd, uint8_t *corr,
                                  int32_t *iters, uint8_t *conv, int64_t B, int32_t threads);

/*
 * OSD under side priors: the OSD half of X/Z-correlated BP+OSD decoding.
 * THE LAW.  An OSD handle (host or GPU) may carry two probability tables p0[n], p1[n], every entry
 * finite and strictly inside (0, 1).  They give two weight tables w_s[j] = log(1 / p_s[j]), computed on
 * the host in double with libm exactly as qldpc_osd_create computes its weights.  A side decode takes
 * side: uint8 [B][n], of which only bit 0 is read.  For syndrome b, a candidate x weighs
 *   sum_{j: x_j = 1} w_{side[b][j] & 1}[j],   the terms added in ascending column order,
 * and the first strictly lightest candidate wins.  The sort, the elimination, OSD-0, the candidate
 * sets and the conv / bp_corr pass-through are those of the plain decode.  A side decode always takes
 * the soft-weight path, even when each table is uniform.  side = 0 everywhere with p0 = the handle's
 * channel_probs is the plain decode bit for bit (a uniform handle's popcount order included: a sum of
 * k equal positive doubles is strictly increasing in k at these n); side = 1 everywhere is the plain
 * decode of a handle built on p1.
 *
 * qldpc_osd_set_side_probs / qldpc_osd_gpu_set_side_probs: QLDPC_EINVAL for an entry outside (0, 1) or
 * non-finite; may be called again to replace the tables; no plain decode changes.  The GPU form may
 * regrow the handle's workspace (it waits for the device first); qldpc_osd_gpu_geometry is unchanged.
 * qldpc_osd_decode_batch_side / qldpc_osd_gpu_decode_side: the plain decodes' arguments with side
 * (d_side on the device); QLDPC_EINVAL when no side tables are set.  The GPU kernels are instantiations
 * of their own (a compile-time switch): they stage the syndrome's n selected weights once in the
 * workgroup's workspace slice, and the candidate walk reads one weight per set bit as the plain
 * non-uniform path does.
 */
int qldpc_osd_set_side_probs(qldpc_osd *osd, const double *p0, const double *p1);
int qldpc_osd_decode_batch_side(const qldpc_osd *osd, const uint8_t *synd, const double *post, const uint8_t *conv,
                                const uint8_t *bp_corr, const uint8_t *side, uint8_t *out_osd0, uint8_t *out_osdw,
                                int64_t B, int32_t threads);
int qldpc_osd_gpu_set_side_probs(qldpc_osd_gpu *osd, const double *p0, const double *p1);
int qldpc_osd_gpu_decode_side(qldpc_osd_gpu *osd, const uint8_t *d_synd, const double *d_post,
                              const uint8_t *d_conv, const uint8_t *d_bp_corr, const uint8_t *d_side,
                              uint8_t *d_out0, uint8_t *d_outw, int64_t B, void *stream);

/*
 * X/Z-correlated decoding in the staged data-error shot loop.  direction: 0 = off, 1 = "x->z", 2 =
 * "z->x".  The X sector is the hz decoder of X components (dec_x), the Z sector the hx decoder (dec_z).
 * Staged handles only (QLDPC_ENOTSUP otherwise; engine-7 and engine-8 decoders land there and
 * qldpc_mc_create_staged forces it); both sector decoders and side tables on the second one are needed
 * (QLDPC_EINVAL otherwise).  With a direction set, qldpc_mc_launch, qldpc_mc_run and
 * qldpc_mc_launch_weight decode the direction's first sector, keep its [B][n] corrections as the side
 * bytes, and decode the second sector with qldpc_bp_decode_batch_side.  Both sectors are then always
 * decoded and their iteration counters tallied, whatever logical_mode; the failure tally (and the
 * per-shot fail bits and sector_fail) follows logical_mode as without a direction.  Sampling, shot
 * keying and the layout of every per-shot output are unchanged.  A handle with a direction set rejects
 * qldpc_mc_set_osd, and a handle with an OSD stage rejects a direction: QLDPC_ENOTSUP.
 */
int qldpc_mc_set_channel_update(qldpc_mc *mc, int32_t direction);

/*
 * BP+OSD in the staged shot loop, with and without a direction.  Staged handles only (QLDPC_ENOTSUP
 * otherwise); each OSD handle must be built on its sector decoder's graph (QLDPC_EINVAL), and the sector
 * decoder must give soft output through qldpc_bp_decode_batch_side_soft (QLDPC_ENOTSUP otherwise: an
 * engine-8 handle created with soft = 1, or an engine-7 handle with num_legs = 0).  NULL clears a sector.
 * With a stage set, qldpc_mc_launch, qldpc_mc_run and qldpc_mc_launch_weight do, per sector: (1) BP with
 * soft output, as a side decode for the second sector of a direction; (2) the GPU OSD over the batch with
 * BP's conv flags, converged decodes keeping BP's correction; (3) outw is the sector's correction: it is
 * what is folded, checked and written to d_corr, and with a direction the first sector's side bytes.
 * With a direction, the second sector's OSD is qldpc_osd_gpu_decode_side on the same side bytes; its
 * side tables are required (QLDPC_EINVAL from whichever of this call and qldpc_mc_set_channel_update
 * comes second).  The iteration and non-converged counters stay BP's: sector_nonconv is the number of
 * decodes handed to OSD.  The posterior buffer is [batch][n] doubles: with a stage set the staged batch
 * is bounded so that it stays within QLDPC_OSD_CAPTURE_MB (default 2048; read as a real number by this
 * call, so a fraction of a megabyte bounds a small code's batch), a multiple of 64, at least 64; shot keying does not depend on the batch, so no result changes with it.  qldpc_mc_set_osd (the
 * fused engine-3 stage) keeps refusing staged handles.
 */
int qldpc_mc_set_staged_osd(qldpc_mc *mc, qldpc_osd_gpu *osd_x, qldpc_osd_gpu *osd_z);

/* BP+OSD in the fused shot loop (bposd_decoder per sector, src/Decoders.py:26-41, inside
 * _single_run, src/Simulators.py:117-168): after qldpc_mc_set_osd, qldpc_mc_launch captures
 * every decode that reaches max_iter (its last-iteration posteriors, syndrome and sampled
 * error) on the device, runs the GPU OSD stage (qldpc_osd_gpu) on those, re-checks their
 * residual against H and the logicals, and corrects the per-shot fail flags and the failure
 * counters -- no host copies beyond the per-sector candidate counts.  Engine-3 MC handles
 * only; each OSD handle must be built on its sector decoder's graph (NULL = plain BP).
 * With an OSD handle set, qldpc_mc_launch is SYNCHRONOUS on its stream (it reads the
 * candidate counts back to size the OSD launch).  Capture memory per sector is bounded by
 * QLDPC_OSD_CAPTURE_MB (default 2048; n*11 + m + 8 bytes per slot); a launch with more shots
 * than slots runs as consecutive pieces, so no candidate is ever dropped. */
int qldpc_mc_set_osd(qldpc_mc *mc, qldpc_osd_gpu *osd_x, qldpc_osd_gpu *osd_z);

/* Engine 3: extra LDS cycles of one variable-phase pass's CS gathers (summed
 * over gather instructions and lane groups: distinct checks on one bank beyond
 * the first) with the identity check order (`before`) and with the labels the
 * decoder uses (`after`, host-side label search at create time; QLDPC_LABEL=0
 * disables it).  0 / 0 for the other engines. */
/* Static LDS model of the engine-3 fp64 variable phase, per workgroup and iteration (zeros for other
 * families): out6 = {CS-gather LDS cycles, of which bank-conflict extra; V-slot read cycles, extra;
 * v2c store group-cycles, extra} under the lane-group rules of MI355X_MICROARCH.md §LDS. */
int qldpc_bp_lds_model(const qldpc_bp *bp, int64_t *out6);
/* The same model for the fp64 m2s family's V-slot placement of graph g, host only (no device, no
 * decoder): the engine's geometry, degree sort, greedy placement and `anneal_iters` annealing moves
 * (< 0 = the default, 4000 per edge; 0 = greedy only).  ENOTSUP outside the m2s envelope. */
int qldpc_m2s_place_model(const qldpc_graph *g, int32_t anneal_iters, int64_t *out6);
int qldpc_bp_bank_stats(const qldpc_bp *bp, int32_t *before, int32_t *after);

/*
 * Multi-GPU.  Shots shard by global index with no data-path
 * exchange; the one collective is the sum of the int64 qldpc_counters vector,
 * which replaces the reference's fork-pool reduction (`parmap` + `np.sum`,
 * src/Simulators.py:37-61 and :170-188).  RCCL (over xGMI) is loaded at first use
 * (dlopen librccl.so.1); without it these return QLDPC_ENOTSUP.
 *   qldpc_comm_unique_id / qldpc_comm_init_rank : one process per GPU (rank 0
 *       makes the id, the host side ships its 128 bytes to every rank);
 *   qldpc_comm_init_all : one process driving ndev GPUs (devices NULL = 0..ndev-1),
 *       out = array of ndev handles;
 *   qldpc_comm_allreduce_counters : in-place sum of a device qldpc_counters on
 *       `stream` (async);
 *   qldpc_comm_allreduce_counters_group : the same for the handles of one
 *       process (qldpc_comm_init_all), one RCCL group call.
 */
#define QLDPC_COMM_ID_BYTES 128
typedef struct qldpc_comm qldpc_comm;
int qldpc_comm_unique_id(uint8_t *id_out);
int qldpc_comm_init_rank(int device, int32_t nranks, int32_t rank, const uint8_t *id, qldpc_comm **out);
int qldpc_comm_init_all(int32_t ndev, const int32_t *devices, qldpc_comm **out);
int qldpc_comm_rank(const qldpc_comm *comm, int32_t *rank, int32_t *nranks, int32_t *device);
int qldpc_comm_allreduce_counters(qldpc_comm *comm, void *d_counters, void *stream);
int qldpc_comm_allreduce_counters_group(qldpc_comm **comms, void **d_counters, void **streams, int32_t n);
int qldpc_comm_destroy(qldpc_comm *comm);

/*
 * `WordErrorRate(num_run)` over several GPUs from ONE host thread
 * (CodeSimulator_DataError.WordErrorRate, src/Simulators.py:170-188, whose
 * `parmap` fans shots out over CPU cores): MC handle d (one per device, each on
 * its own device's decoders) runs a contiguous block of the global shots (block
 * sizes S/ndev or S/ndev + 1, the first S%ndev devices one longer: the split of
 * parallel.shard_range), the counters are summed
 * with one grouped all-reduce (comms from qldpc_comm_init_all, in the same
 * device order: comms[d] must be rank d of ndev, on MC handle d's device, else
 * QLDPC_EINVAL; per-process qldpc_comm_init_rank communicators are refused) or,
 * with comms NULL, on the host; the sum is added to *out.  Each device is
 * driven from its own host thread (BP+OSD launches are synchronous).
 * Synchronous.  The ndev > 1 RCCL path has not yet run on a multi-GPU node.
 * Shots keyed by global index: the totals do not depend on ndev.
 */
/* The shot-block split qldpc_mc_run_sharded uses (= parallel.shard_range): part `part` of `nparts`
 * owns [begin, begin + count) of `total` shots, block sizes differ by <= 1, the first total % nparts
 * parts one longer.  Host-only (no GPU needed). */
int qldpc_shard_range(int64_t total, int32_t nparts, int32_t part, int64_t *begin, int64_t *count);
int qldpc_mc_run_sharded(qldpc_mc **mcs, qldpc_comm **comms, int32_t ndev, double px, double py, double pz,
                         uint64_t seed, uint64_t shot_begin, int64_t shot_count, int32_t logical_mode,
                         qldpc_counters *out);

/*
 * Circuit-level space-time shot loop (CodeSimulator_Circuit_SpaceTime._single_run / WordErrorRate,
 * src/Simulators_SpaceTime.py:968-1049) for many samples per launch.  Inputs (host CSR graphs
 * from qldpc_graph_create; qldpc_fault_tolerance_amd/circuit.py builds them):
 *   dem, dem_obs : detectors x mechanisms / observables x mechanisms of the FULL circuit's DEM
 *                  (the stim detector_sampler's distribution, :940; rows = num_cycles * m
 *                  detectors, num_cycles = num_rounds * num_rep + 1), probs [M] host doubles;
 *   dec1         : decoder1 on h1 (num_rep * m rows; GenFaultHyperGraph's first layer, :955);
 *   h1_space_cor : GenCorrecHyperGraph (m x n1), L1 (K x n1) the first layer's observables;
 *   dec2, L2     : decoder2 on h2 (m x n2) and the last layer's observables.
 * Sample s draws mechanism j when Philox4x32-10(key = seed, ctr = (j, shot, 0x51D50003)) as a
 * 53-bit uniform is < probs[j] (shot = shot_begin + s).  Counters: shots, failures, sector 0 =
 * decoder1 decodes (num_rounds per sample), sector 1 = decoder2 decodes.  d_fail [S] (or NULL),
 * d_detobs [S][D + K] sampled detector and observable bits (or NULL).  Asynchronous on `stream`
 * (no host round trip, BP+OSD included, unless the OSD is a host stage past the GPU envelope).  dec1 = dec2 = NULL (and NULL h1_space_cor / L1 /
 * L2) makes a sampler-only handle for qldpc_circ_sample (decoders outside the engine).
 */
typedef struct qldpc_circ qldpc_circ;
int qldpc_circ_create(const qldpc_graph *dem, const qldpc_graph *dem_obs, const double *probs, qldpc_bp *dec1,
                      const qldpc_graph *h1_space_cor, const qldpc_graph *L1, qldpc_bp *dec2, const qldpc_graph *L2,
                      int32_t num_rounds, int32_t num_rep, int64_t max_batch, qldpc_circ **out);
/*
 * Single-shot mode of the same handle: CodeSimulator_Circuit._decoding_samples (src/Simulators.py:612-644)
 * on the DEM of the single-shot circuit (num_cycles * m detectors, cycle-major; circuit.py
 * single_shot_circuit).  Per sample, hist[j] = detector rows j * m .. j * m + m - 1:
 *   res = 0;  for j in 0 .. num_cycles - 2:  s = hist[j] ^ res;  c = decoder1(s);
 *                                             res = s ^ h_space c;  logical ^= L1 c;
 *   s_f = hist[num_cycles - 1] ^ res;  c2 = decoder2(s_f);
 *   failure = (s_f ^ h2 c2 != 0) or (observables ^ logical ^ L2 c2 != 0).
 *   dec1    : decoder1 on [hx | I] (m x n1, n1 = n + m), or NULL (below);
 *   h_space : m x n1 = [hx | 0]: the identity (syndrome-error) part of a correction is NOT applied;
 *   L1      : K x n1 = [lx | 0];  dec2, L2 : decoder2 on h2 (m x n2) and K x n2 (= lx on hx).
 * One cycle = one step kernel (residual and logical carry from the previous correction, this
 * cycle's detector words, the next decode's syndrome bytes), the decode, its statistics.  The handle
 * works with qldpc_circ_launch / _sample / _set_final_osd / _set_sampler / _info / _destroy; counters:
 * sector 0 = decoder1 decodes (num_cycles - 1 per sample), sector 1 = decoder2 decodes; d_fail and
 * d_detobs as above.  Asynchronous, shard- and batch-invariant.  QLDPC_EINVAL: num_cycles < 2,
 * D != num_cycles * m, decoder1 not m x n1, mismatched shapes or devices.
 *
 * qldpc_circ_set_round_firstmin makes the rounds decode with a FirstMinBPDecoder handle (the
 * Single-Shot notebook's decoder1 on [h | I]) instead of dec1; accepted steps count as iterations
 * and no decode counts as non-converged, as in qldpc_phenl_set_round_firstmin.  The handle must be
 * built on exactly decoder1's graph.  With dec1 = NULL at creation that graph is [hx | I] as h_space
 * gives it (row r = h_space's row r and column n1 - m + r), and qldpc_circ_launch returns
 * QLDPC_EINVAL until a first-min handle is set; fm = NULL goes back to dec1 (QLDPC_EINVAL when there
 * is none).  QLDPC_EINVAL on a space-time handle.  The caller keeps fm alive while it is set.
 */
int qldpc_circ_create_single_shot(const qldpc_graph *dem, const qldpc_graph *dem_obs, const double *probs,
                                  qldpc_bp *dec1, const qldpc_graph *h_space, const qldpc_graph *L1, qldpc_bp *dec2,
                                  const qldpc_graph *L2, int32_t num_cycles, int64_t max_batch, qldpc_circ **out);
int qldpc_circ_set_round_firstmin(qldpc_circ *circ, qldpc_firstmin *fm);
/* decoder2 as bposd_decoder (ST_BPOSD_Decoder_Circuit, src/Decoders_SpaceTime.py:277-292): dec2 from
 * qldpc_bp_create_soft and ONE of a GPU OSD or a host OSD stage on h2; a host stage is turned into a
 * GPU OSD with its method, order, rank and soft weights, so the launch never leaves the device —
 * except past the GPU kernel's envelope (n > 8192; osd_e stops at order 20 in both stages), where the host stage decodes
 * the final layer (one synchronous D2H / H2D round trip per batch inside qldpc_circ_launch). */
int qldpc_circ_set_final_osd(qldpc_circ *circ, qldpc_osd_gpu *osd_gpu, const qldpc_osd *osd_host);
/* DEM sampler of qldpc_circ_launch / qldpc_circ_sample (stim's compile_detector_sampler().sample,
 * src/Simulators_SpaceTime.py:940, :1029): 1 = geometric skip (the default since round 6: per
 * mechanism and global 64-sample word, Philox-drawn gaps u < ceil(2^53 (1 - p)^k); ~1 + 64 p draws
 * per word), 0 = keyed (one Philox uniform per (sample, mechanism), u < p).  Both are exact
 * Bernoulli(p_j) samplers keyed by global sample indices (shard-invariant); they draw different
 * samples. */
int qldpc_circ_set_sampler(qldpc_circ *circ, int32_t sampler);
int qldpc_circ_info(const qldpc_circ *circ, int32_t *detectors, int32_t *observables, int32_t *mechanisms);
int qldpc_circ_launch(qldpc_circ *circ, uint64_t seed, uint64_t shot_begin, int64_t shot_count, void *d_counters,
                      uint8_t *d_fail, uint8_t *d_detobs, void *stream);
/* The sampling step alone (stim's detector sampler): d_out [S][D + K] uint8 detector then
 * observable bits of samples shot_begin.. (the draws qldpc_circ_launch decodes).  Async. */
int qldpc_circ_sample(qldpc_circ *circ, uint64_t seed, uint64_t shot_begin, int64_t shot_count, uint8_t *d_out,
                      void *stream);
int qldpc_circ_destroy(qldpc_circ *circ);

/*
 * The sampling step alone (CodeSimulator_DataError._generate_error,
 * src/Simulators.py:89-115): d_err uint8 [S][n], bit0 = x, bit1 = z, from the
 * Philox stream of qldpc_mc_launch (shot shot_begin + s, qubit j) or from
 * d_uniforms [S][n] (CPython's random() values) with the reference's 3-way
 * split.  Bit-identical to the d_err output of qldpc_mc_launch.  Async.
 */
int qldpc_sample_errors(double px, double py, double pz, uint64_t seed, uint64_t shot_begin, int64_t shot_count,
                        int32_t n, const double *d_uniforms, uint8_t *d_err, void *stream);

/*
 * The fixed-weight sampler of qldpc_mc_launch_weight alone: d_err uint8 [S][n], bit0 = x, bit1 = z,
 * exactly `weight` non-zero entries per row; bit-identical to that call's d_err output.  Async.
 * The _host form is the same law in plain C++ on host memory (no HIP call, any n).
 */
int qldpc_sample_errors_weight(int32_t weight, double px, double py, double pz, uint64_t seed, uint64_t shot_begin,
                               int64_t shot_count, int32_t n, uint8_t *d_err, void *stream);
int qldpc_sample_errors_weight_host(int32_t weight, double px, double py, double pz, uint64_t seed,
                                    uint64_t shot_begin, int64_t shot_count, int32_t n, uint8_t *err);

/*
 * Random information-set minimum-distance search (distance.hip): what replaces the reference's
 * compute_code_distance(H) / hgp(..., compute_distance=True) (src/QuantumExanderCodesGene.py) at sizes
 * where enumeration is impossible.  gen_words: a generator matrix of the kernel of a check matrix, rows x n
 * bits packed 64 columns per uint64 word (bit c & 63 of word c >> 6), row-major; pair_words: its pairing
 * G L^T with the k logical operators of the other sector, packed the same way, or NULL with k = 0 for a
 * classical code.  Trial t orders the columns by ascending (key, c), key = first word of Philox4x32-10 at
 * counter (c, t_lo, t_hi, 0x51D50005) and key (seed_lo, seed_hi), runs a greedy Gauss-Jordan in that
 * order and reports min (weight, pivot position) over the rows that hold a pivot and have non-zero
 * pairing; a range reports min (weight, trial), that row (n bits, original column numbering) and the
 * per-trial minima (0x7FFFFFFF: no candidate).  Results are independent of the grid and of how a
 * range is cut into calls.  device = -1: host-only handle (no HIP call, any size); a device handle
 * needs 1 <= rows <= 1024 and at most 28 row words, code plus pairing (QLDPC_ENOTSUP otherwise).
 * Outputs are host memory; qldpc_dist_run synchronizes `stream`.  workgroups = 0: compute units x
 * (1024 / threads) workgroups, 1024 threads' worth per compute unit (LDS may keep fewer resident;
 * the trial loop is grid-strided, so residency is not needed).
 */
typedef struct qldpc_dist qldpc_dist;
int qldpc_dist_create(int device, int32_t rows, int32_t n, int32_t k, const uint64_t *gen_words,
                      const uint64_t *pair_words, qldpc_dist **out);
int qldpc_dist_run_host(qldpc_dist *h, uint64_t seed, uint64_t trial_begin, int64_t trials, int32_t *trial_min,
                        int32_t *best_weight, uint64_t *best_trial, uint64_t *witness_words);
int qldpc_dist_run(qldpc_dist *h, uint64_t seed, uint64_t trial_begin, int64_t trials, int32_t workgroups,
                   int32_t *trial_min, int32_t *best_weight, uint64_t *best_trial, uint64_t *witness_words,
                   void *stream);
/* threads per workgroup, code words and pairing words per row, LDS bytes (0 threads / bytes: host handle) */
int qldpc_dist_geometry(const qldpc_dist *h, int32_t *threads, int32_t *row_words, int32_t *pair_words,
                        int32_t *lds_bytes);
int qldpc_dist_destroy(qldpc_dist *h);

/* hipStreamSynchronize(stream) for hosts without a HIP binding (NULL = legacy default stream). */
int qldpc_stream_sync(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QLDPC_HIP_H */
