/*
 * cdr.h — C ABI of the MI355X (gfx950) clustering hot path.
 *
 * "cdr" = clustering-driven replication.  One shared library, libcdr.so, built
 * from hand-written HIP kernels.  Every entry point takes plain pointers and
 * sizes and returns an int status (CDR_OK == 0).  On failure the message is
 * available from cdr_last_error() (thread-local).
 *
 * The reference (Harounnn/Clustering-Driven-Replication-Strategy) has no FFI:
 * its hot path is NumPy / PySpark code.  Each block below names the reference
 * function it replaces (file:line relative to the reference root).  The Python
 * drop-in modules (kmeans_plusplus.py, scoring.py, compute_features.py) bind
 * these symbols through ctypes; INTEGRATION.md shows the binding.
 *
 * Ownership: host pointers belong to the caller and are only read/written for
 * the duration of the call.  Device buffers belong to the context.  A context
 * is bound to one HIP device and is NOT thread-safe (the reference is
 * single-threaded and uses global NumPy RNG state, src/kmeans_plusplus.py:43).
 * All calls are synchronous from the caller's point of view unless the name
 * ends in _async.
 */
#ifndef CDR_H_
#define CDR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define CDR_OK 0
#define CDR_ERR_ARG 1         /* bad argument  -> Python ValueError            */
#define CDR_ERR_HIP 2         /* HIP runtime    -> Python RuntimeError          */
#define CDR_ERR_NAN 3         /* NaN probabilities (kmeans_plusplus.py:18-19)   */
#define CDR_ERR_STATE 4       /* call order     -> Python RuntimeError          */
#define CDR_ERR_UNSUPPORTED 5 /* shape not supported -> NotImplementedError     */

/* ---- point storage modes (cdr_points_info) ----------------------------- */
/* F32X: every coordinate is an fp32 value on a 2^-S grid with |x|*2^S < 2^31.
 *       Screen + exact fallback assignment; centroid sums are exact int64
 *       fixed point (bit-identical to NumPy's sequential fp64 mean whenever
 *       that mean is itself exact, e.g. 2^-24-grid data).                     */
#define CDR_MODE_F32X 1
/* F64:  arbitrary fp64 data.  Exact fp64 assignment for every point and
 *       sequential per-cluster fp64 sums in row order (NumPy mean order).     */
#define CDR_MODE_F64 2

typedef struct cdr_ctx cdr_ctx;

const char* cdr_last_error(void);
int cdr_version(void);
int cdr_device_count(int* out);

/* Context on HIP device `device`.  Owns a HIP stream unless one is supplied
 * with cdr_set_stream (e.g. torch.cuda.current_stream().cuda_stream).       */
int cdr_create(int device, cdr_ctx** out);
int cdr_destroy(cdr_ctx* ctx);
int cdr_set_stream(cdr_ctx* ctx, void* hip_stream);
int cdr_synchronize(cdr_ctx* ctx);

/* ---- point set (the X of src/main.py:81, one shard per context) -------- */
/* Host row-major float64 (n, d).  Detects the storage mode (see above).     */
int cdr_points_load_f64(cdr_ctx* ctx, const double* X, int64_t n, int32_t d);
/* Synthetic generator (BASELINE configs 2/3/5): rows [row_begin, row_begin +
 * n_local) of an n_total-row data set, generated on the device.  Integer-only
 * counter-based formula; oracle/synth.py is the NumPy mirror.               */
int cdr_points_generate(cdr_ctx* ctx, int64_t n_total, int64_t row_begin,
                        int64_t n_local, int32_t d, int32_t n_blobs,
                        uint64_t seed);
int cdr_points_info(cdr_ctx* ctx, int64_t* n, int32_t* d, int32_t* mode,
                    int32_t* scale_bits);
/* Points sharded over ranks: every rank must use the same
 * storage mode, fixed-point scale S and screen transform, or the int64 sums
 * of the all-reduce and the device loop's stop decisions would differ per
 * rank.  cdr_points_stats: this shard's statistics st[2d + 3] (uint64 order
 * keys of the per-feature minima, then maxima; max(-lsb) + 200000; not-fp32
 * flag; non-finite flag).  cdr_points_restat: re-decide mode / S / transform
 * from statistics combined over every shard (MIN of the minimum keys, MAX of
 * every other word) and the global row count n_sum.                         */
int cdr_points_stats(cdr_ctx* ctx, uint64_t* st);
int cdr_points_restat(cdr_ctx* ctx, const uint64_t* st, int64_t n_sum);
/* Copy local rows idx[0..m) to host as float64 (m, d). */
int cdr_points_get_rows(cdr_ctx* ctx, const int64_t* idx, int64_t m,
                        double* out);

/* ---- k-means++ D^2 seeding: src/kmeans_plusplus.py:3-22 ---------------- */
/* dist_sq := +inf (before the first centre).                                */
int cdr_seed_reset(cdr_ctx* ctx);
/* dist_sq[i] = min(dist_sq[i], (sqrt(pw_d((x_i - c)^2)))^2), NumPy order
 * (kmeans_plusplus.py:14-17), then the 8192-element pairwise block sums of
 * dist_sq (NumPy's blocked add.reduce, used by dist_sq.sum() at :18).  c is
 * one float64 row of length d.                                              */
int cdr_seed_update(cdr_ctx* ctx, const double* c);
/* The reference's float32 seeding step (src/kmeans_plusplus.py:14-18 on a
 * float32 X): dist_sq = min(dist_sq, fp32(norm(X - c))**2) with c float32
 * (reset != 0: dist_sq starts at +inf), *total = dist_sq.sum() in fp32
 * (NumPy's 8192-chunk pairwise order), and the probabilities fp32(dist_sq /
 * total) staged as doubles for cdr_seed_scan(ctx, 1.0, ...) and
 * cdr_seed_search, which then give rng.choice's pick.  CDR_ERR_NAN when the
 * total is not positive and finite.                                        */
int cdr_f32r_seed_update(cdr_ctx* ctx, const float* c, int32_t reset, float* total);
/* Number of 8192-element blocks of this shard and their pairwise sums.     */
int cdr_seed_num_blocks(cdr_ctx* ctx, int64_t* nblocks);
int cdr_seed_block_sums(cdr_ctx* ctx, double* out);
/* Exact sequential cumulative sum of probs = dist_sq / total over this
 * shard, starting from running value c_in (0.0 on the first shard); returns
 * the running value after the shard's last element.  Emulates np.cumsum
 * bit-exactly (Generator.choice, kmeans_plusplus.py:19).                   */
int cdr_seed_scan(cdr_ctx* ctx, double total, double c_in, double* c_out);
/* The same scan in two halves, for sharded seeding without a rank-ordered
 * chain (cdr_dist.seed_sharded replaces kmeans_plusplus.py:19's single
 * np.cumsum over all rows).  _begin builds this shard's cumsum program from
 * a GUESS of the running value at its first element (the sum of the earlier
 * shards' block sums / total); the program is the shard's exact function
 * c_in -> c_out as long as it has no CDR_SEED_FINE item.  _items copies it
 * out; cdr_seed_program_eval runs it on the host (no device, no context).
 * _end takes the exact c_in, fills what cdr_seed_search needs and returns
 * c_out — exact whatever the guess was (it falls back to the block walk).  */
typedef struct {
  int64_t d0, d1; /* RUN: grid steps added for an even / odd entry         */
  double p;       /* CROSS: the element added; CONST: the value            */
  int32_t e;      /* RUN: binade exponent                                   */
  int32_t kind;   /* CDR_SEED_*                                             */
} cdr_seed_item;
enum {
  CDR_SEED_RUN = 0,   /* c in binade e: N += (N odd ? d1 : d0), N < 2^53    */
  CDR_SEED_CROSS = 1, /* c = fl(c + p)                                      */
  CDR_SEED_CONST = 2, /* c = p (a shard whose c_in is known: the first)     */
  CDR_SEED_FINE = 3,  /* element walk of block d0 (device only)             */
  CDR_SEED_MARK = 4,  /* device bookkeeping; no-op                          */
  CDR_SEED_END = 5,
  CDR_SEED_SKIP = 6,  /* empty run                                          */
  CDR_SEED_BAD = 7    /* the guess cannot hold: evaluation fails            */
};
int cdr_seed_scan_begin(cdr_ctx* ctx, double total, double c_guess, int64_t* n_items,
                        int64_t* n_fine);
int cdr_seed_scan_items(cdr_ctx* ctx, cdr_seed_item* out, int64_t cap, int64_t* n_items);
int cdr_seed_scan_end(cdr_ctx* ctx, double c_in, double* c_out);
/* out[0] = scans run through a program, out[1] = of those, the ones whose
 * guess failed and fell back to the exact block walk (same result; counted
 * by the per-step calls — cdr_seed_run gates its fallback on the device).  */
int cdr_seed_stats(cdr_ctx* ctx, int64_t* out);
/* The whole kmeans_plusplus_init (:3-22) on this context's points with no host
 * round trip per step: first = the first row (rng.integers), u[0..k-1) = the
 * uniforms of the k - 1 draws (rng.choice takes one rng.random() each);
 * picks[0..k) = the chosen rows.  CDR_ERR_NAN when a total is not finite and
 * positive ("Probabilities contain NaN").                                   */
int cdr_seed_run(cdr_ctx* ctx, int64_t first, int32_t k, const double* u, int64_t* picks);
/* The reference's float32 seeding (src/kmeans_plusplus.py:3-22 on a float32
 * X, the semantics of cdr_f32r_seed_update) as one device-resident run, like
 * cdr_seed_run: fp32 dist_sq, totals and probabilities, rng.choice's pick per
 * step on the device.  CDR_ERR_NAN as cdr_f32r_seed_update, with the message
 * "probabilities do not sum to 1" (Generator.choice's) when a total overflows
 * to +inf while every dist_sq is finite.                                    */
int cdr_f32r_seed_run(cdr_ctx* ctx, int64_t first, int32_t k, const double* u, int64_t* picks);
/* The same over rows sharded across nranks ranks (whole 8192-row blocks per
 * shard, this context holding rows [row_begin, row_begin + n) of n_total),
 * device-resident: per step three phases, each followed by one collective the
 * caller runs on device buffers —
 *   begin            -> red (d + 4 doubles): SUM all-reduce
 *   phase 0 (red)    -> this rank's slot of the block sums [nranks][nbmax]:
 *                       all-gather
 *   phase 1 (sums)   -> this rank's slot of the programs [nranks][1024 items]:
 *                       all-gather
 *   phase 2 (progs)  -> red: SUM all-reduce
 * (k - 1 steps), then end (red) -> picks[0..k) (global rows), centres (k x d
 * fp64, the picked rows: every rank has them), status 0 ok,
 * 1 "run the host protocol instead" (a program could not be composed, or
 * disagreed with its own scan: seen by every rank through the all-reduce),
 * 2 a total not finite and positive (Probabilities contain NaN).  sizes[3]:
 * bytes per rank of the three buffers.  cdr_seed_run_sharded runs every step
 * with the context's communicator (cdr_comm_init).  Reference:
 * src/kmeans_plusplus.py:3-22.                                               */
int cdr_seed_shard_begin(cdr_ctx* ctx, int64_t row_begin, int64_t n_total, int32_t nranks,
                         int32_t rank, int64_t first, int32_t k, const double* u, double* red,
                         int64_t* sizes);
int cdr_seed_shard_phase(cdr_ctx* ctx, int32_t phase, const void* in, void* out);
int cdr_seed_shard_end(cdr_ctx* ctx, const double* red, int64_t* picks, double* centres,
                       int32_t* status);
int cdr_seed_run_sharded(cdr_ctx* ctx, int64_t row_begin, int64_t n_total, int64_t first, int32_t k,
                         const double* u, int64_t* picks, double* centres, int32_t* status);
/* *ok = 0 when some item does not hold for this c_in (or a FINE item).      */
int cdr_seed_program_eval(const cdr_seed_item* items, int64_t n_items, double c_in,
                          double* c_out, int32_t* ok);
/* searchsorted(cumsum / c_last, u, side='right') restricted to this shard:
 * *idx = local index, or -1 when the crossing is not in this shard.        */
int cdr_seed_search(cdr_ctx* ctx, double c_last, double u, int64_t* idx);

/* ---- Lloyd iteration: src/kmeans_plusplus.py:31-43 --------------------- */
/* One assignment + fused update pass for centroids C (k, d) float64.
 * Labels stay on the device (cdr_lloyd_labels).
 * F32X mode: out (k, d+1) int64 = per-cluster fixed-point sums (value *
 *   2^scale_bits) and counts in column d.  `out_on_device` != 0 means `out`
 *   is a device pointer on this context's device; the kernels then write it
 *   on the context stream without synchronising (for an RCCL all-reduce).
 * F64 mode: use cdr_lloyd_step_f64.                                          */
int cdr_lloyd_step(cdr_ctx* ctx, const double* C, int32_t k, int64_t* out,
                   int32_t out_on_device);
/* F64 mode: exact fp64 assignment; sums (k, d) float64 accumulated in row
 * order exactly like X[labels == j].mean(axis=0)'s sum; counts (k).        */
int cdr_lloyd_step_f64(cdr_ctx* ctx, const double* C, int32_t k, double* sums,
                       int64_t* counts);
/* F64 mode, 2 <= d <= 16, k <= 64: up to max_steps Lloyd steps resident on
 * the device (src/kmeans_plusplus.py:31-48; replaces a host loop of
 * cdr_lloyd_step_f64 + means + shift): each step's exact assignment and
 * sequential sums, then means = sums / counts and shift = ||means - C|| on
 * the device.  info[0] = steps applied (C replaced by the means); info[1] =
 * 0 all max_steps applied, 1 converged (the last applied step had shift <
 * tol), 2 the next step needs the host (an empty cluster, or a shift too
 * close to tol to decide): that step is NOT applied, C_out is the centroids
 * it started from, means_out (k, d) / counts_out (k) are its means and
 * counts, and the labels on the device are its assignment.  C_out (k, d):
 * the centroids after the applied steps.  tol <= 0: never converges.      */
int cdr_lloyd_f64_run(cdr_ctx* ctx, const double* C, int32_t k, int32_t max_steps, double tol,
                      double* C_out, double* means_out, int64_t* counts_out, int32_t* info);
/* The reference's float32 runs (X float32 keeps its dtype,
 * src/kmeans_plusplus.py:6, 33-34, 41): float32 norms in NumPy order, argmin
 * of the fp32 norms, sums (k, d) = the SEQUENTIAL float32 sums of each
 * cluster's rows (returned as doubles holding fp32 values; the caller
 * divides in fp64 and casts to fp32, as np.mean does); counts (k).
 * C: k x d float32.  Points loaded from a float32 array (either mode).  */
int cdr_lloyd_step_f32r(cdr_ctx* ctx, const float* C, int32_t k, double* sums,
                        int64_t* counts);
/* F64 mode, d >= 2, k <= 64: the sums are formed in parallel (csrc/f64sum.hip:
 * per-block parity transfers inside one binade, exact); *walked = blocks of
 * (cluster, feature) sequences re-added element by element in the last step,
 * or -1 when the step used the serial kernel.                               */
int cdr_lloyd_f64_walked(cdr_ctx* ctx, int64_t* walked);
/* Sharded F64 sums (src/kmeans_plusplus.py:33-41 on rows sharded in rank
 * order, float64 data off any grid: src/main.py:81).  Per Lloyd step, with
 * one collective between the calls (buffers are device memory: all ranks'
 * slots, rank r's at offset r x its slot size):
 *   cdr_f64s_begin   assignment (labels) + this shard's approximate
 *                    per-(cluster, feature) totals and member counts into
 *                    its slot of tot_buf; sizes = {tot slot bytes, program
 *                    slot bytes}                       -> all-gather tot_buf
 *   cdr_f64s_build   this shard's program (rank 0: its exact walked sums;
 *                    rank > 0: transfer runs and element lists built from
 *                    the gathered approximate totals) -> all-gather prog_buf
 *   cdr_f64s_finish  every rank composes all programs in rank order: the
 *                    exact sequential sums (k x d) and counts (k); *status
 *                    1 when a program's guess did not hold, the same on
 *                    every rank: then run the rank chain, cdr_f64s_chain on
 *                    rank r (walks its shard from the exact entry
 *                    chain_buf[0, 2 k d) = {sums, any}, leaving its exit
 *                    there) followed by a broadcast of chain_buf from rank r,
 *                    for r = 0 .. nranks - 1 (chain_buf zeroed first).
 * Replaces the sequential NumPy mean (kmeans_plusplus.py:41) over the whole
 * array; 2 <= d <= 16, k <= 64.                                            */
int cdr_f64s_begin(cdr_ctx* ctx, const double* C, int32_t k, int32_t nranks, int32_t rank,
                   void* tot_buf, int64_t* sizes);
int cdr_f64s_build(cdr_ctx* ctx, const void* tot_buf, void* prog_buf);
int cdr_f64s_finish(cdr_ctx* ctx, const void* tot_buf, const void* prog_buf, double* sums,
                    int64_t* counts, int32_t* status);
int cdr_f64s_chain(cdr_ctx* ctx, void* chain_buf);
/* Labels of the last assignment as int64 (np.argmin dtype, :34).           */
int cdr_lloyd_labels(cdr_ctx* ctx, int64_t* labels);
/* Diagnostics of the last step: points the fast screen could not certify
 * and that went through the exact fp64 path.                                */
int cdr_lloyd_stats(cdr_ctx* ctx, int64_t* n_fallback);
/* Profiling: enable != 0 starts collecting HIP-event timings of every
 * enable-th following F32X step (1: every step; the event records cost the GPU
 * a few microseconds each) on the context stream; cdr_profile_read returns
 * out[6] = {screen kernel ms (sum), steps, whole step kernels ms (sum),
 * fallback points (sum), points the pruned screen queued for its k-way MFMA
 * screen (sum), points whose drift bound failed in the bounded screen and were
 * re-decided from their coordinates (sum)}.                                  */
int cdr_profile_reset(cdr_ctx* ctx, int32_t enable);
int cdr_profile_read(cdr_ctx* ctx, double* out);
/* The same session's steps whose screen ran as two kernels (the split bounded
 * screen: screen32bz, then screen32bs): out[2] = {ms from the step start to
 * the end of the first kernel (sum), such steps}.                            */
int cdr_profile_read_sub(cdr_ctx* ctx, double* out);

/* ---- device-resident Lloyd loop: src/kmeans_plusplus.py:31-48 ----------- */
/* The same iterations as cdr_lloyd_step + the host's means / reseed / shift,
 * but the means, the shift and the convergence test run on the device
 * (bit-identical: the same fp64 operations), so steps can be enqueued without
 * a host round trip.  The device STOPS the loop (later enqueued steps do
 * nothing) and reports why whenever the reference's host logic is needed:
 * an empty cluster (np.random.randint reseed, :43), a shift within 1e-9
 * relative of tol (np.linalg.norm decides, :45-47), or centroids outside the
 * fp16 screen range.  F32X points only (CDR_ERR_UNSUPPORTED otherwise).
 *
 * cdr_points_sqdev: sum_i ||x_i - ref||^2 (fp64) of this shard; with ref a
 *   data row this is exact per term; it anchors the inertia.
 * cdr_lloyd_begin: centroids C (k, d); tol (<= 0: never converged); flags bit
 *   0: round the means to float32 (X is float32); ref (d) and x2_total =
 *   cdr_points_sqdev summed over every shard (NaN: this shard alone).
 * cdr_lloyd_enqueue_assign: assignment + fused update of the current
 *   centroids; the (k, d+1) int64 sums go to dsums (device pointer, e.g. the
 *   buffer an RCCL all-reduce sums next) or to an internal buffer (NULL).
 * cdr_lloyd_enqueue_finalize: means / shift / inertia from the (all-reduced)
 *   sums at dsums (NULL: the internal buffer) and the move to the means.
 * cdr_lloyd_status (synchronises): status[4] = {running, steps done, stop
 *   reason (0 running, 1 converged, 2 empty cluster, 3 needs the host plan,
 *   4 shift too close to tol), steps enqueued}; values[2] = {shift, inertia}
 *   of the last finalised step.
 * cdr_lloyd_read: current centroids C (k, d), the last means (k, d, NaN rows
 *   for empty clusters) and counts (k); any pointer may be NULL.
 * cdr_lloyd_resume: after the host took a step itself: C (NULL keeps the
 *   device's), add_steps to the step count, host_plan_once != 0 runs the next
 *   assignment on the host-plan path.                                      */
int cdr_points_sqdev(cdr_ctx* ctx, const double* ref, double* out);
int cdr_lloyd_begin(cdr_ctx* ctx, const double* C, int32_t k, double tol, int32_t flags,
                    const double* ref, double x2_total);
int cdr_lloyd_enqueue_assign(cdr_ctx* ctx, int64_t* dsums);
int cdr_lloyd_enqueue_finalize(cdr_ctx* ctx, const int64_t* dsums);
int cdr_lloyd_status(cdr_ctx* ctx, int64_t* status, double* values);
int cdr_lloyd_read(cdr_ctx* ctx, double* C, double* means, int64_t* counts);
int cdr_lloyd_resume(cdr_ctx* ctx, const double* C, int32_t add_steps, int32_t host_plan_once);
int cdr_lloyd_end(cdr_ctx* ctx);
/* m loop steps enqueued by one call: assign, the SUM all-reduce of the
 * (k, d+1) int64 sums over the context's communicator (cdr_comm_init; none:
 * a single shard), finalize — no host synchronisation and no host code
 * between a step's kernels and its collective.                              */
int cdr_lloyd_enqueue_steps(cdr_ctx* ctx, int32_t m);

/* ---- native collective for the loop: RCCL over xGMI ------------------- */
/* One communicator per context (one process per GPU).  cdr_comm_unique_id
 * writes the 128-byte ncclUniqueId (one rank creates it, the caller
 * broadcasts it); cdr_comm_init joins the nranks-rank communicator as `rank`
 * on the context's device; cdr_comm_destroy leaves it.  librccl is bound at
 * run time; CDR_ERR_UNSUPPORTED when it cannot be loaded.                   */
int cdr_comm_unique_id(void* id128);
int cdr_comm_init(cdr_ctx* ctx, const void* id128, int32_t nranks, int32_t rank);
int cdr_comm_destroy(cdr_ctx* ctx);
/* *ok = 1 when librccl loads and has the entry points (dlopen / dlsym only:
 * unlike cdr_comm_unique_id it starts no bootstrap listener, so every rank may
 * probe with it).                                                            */
int cdr_comm_available(int32_t* ok);
/* The context's communicator: *nranks (0 when it has none) and *rank.       */
int cdr_comm_ranks(cdr_ctx* ctx, int32_t* nranks, int32_t* rank);
/* Name of the last screen kernel launched (for the bench's roofline line);
 * NUL-terminated, truncated to len.                                          */
int cdr_profile_kernel(cdr_ctx* ctx, char* buf, int32_t len);
/* Work distribution of the context's last bounded-screen launch (tests):
 * out = {workgroups, workgroups per generation region (0: one strided split),
 * the dynamic tail's static percent (100: off), the most chunks a wave streams
 * statically, chunks, bytes per bound word (2 or 4)}; all zeros when no
 * bounded screen has run on the context.                                    */
int cdr_lloyd_screen_layout(cdr_ctx* ctx, int32_t out[6]);
/* The watch list of the 2-byte bounded screen after the context's last step
 * (tests; synchronises the stream): out = {mode of the last
 * screen (1: it streamed the list, 0: every word, -1: the list path is off or
 * no screen has run with it), entries listed by the last build, entries (mode
 * 1) or words (mode 0) that failed in the last screen, lists built, screens
 * that streamed every word while the list path was on, screens that streamed
 * the list, waves, points per wave, entries a wave's region holds, 1 when the
 * next screen would stream the list, lists built in the pass that carried a
 * rebase of the words, padded points (the bound words the context keeps)}.   */
int cdr_lloyd_watch_info(cdr_ctx* ctx, int64_t out[12]);
/* Test hook: the n_words bound words (2 bytes each), the watch list's
 * n_entries region entries (waves x entries per region,
 * offset_in_wave_range << 16 | word), the regions' lengths (waves) and the
 * code tables T | H | H of the list's build (3 x 64); any pointer may be
 * null.  An error while the list path is off, or when n_words or n_entries
 * differ from the padded points or waves x entries per region that
 * cdr_lloyd_watch_info reports.                                              */
int cdr_debug_watch(cdr_ctx* ctx, uint16_t* words, int64_t n_words, uint32_t* entries,
                    int64_t n_entries, int32_t* counts, uint32_t* tables);
/* What the context's last large-k step (screen_big.hip) chose and counted
 * (tests): out = {DQ = ceil(d/16), KB = ceil(k/32), FG (features per update
 * pass), JB (key bits holding the centroid index), L1 threads (512 or 768),
 * L2 form (0: cand_big_lds, 1: cand_big), delta (0: full update pass, 1: moves
 * only), plan (0: host, 1: device), L1 regions, capacity of a region, 64-point
 * groups, L1 leftovers, points L3 decided, moves L1 recorded, moves L2 and L3
 * recorded}; all zeros when no large-k step has run since the points were
 * loaded.  The four counters are read back here, after a stream synchronise,
 * from the step's own buffers: ask before the next step reuses them.         */
int cdr_lloyd_big_layout(cdr_ctx* ctx, int64_t out[15]);
/* Test hook (not product path): screen values T (n_pad, ceil(k/16)*16) fp32
 * of one F32X step and the certification constants (A0, A1).               */
int cdr_debug_screen(cdr_ctx* ctx, const double* C, int32_t k, float* out_vals,
                     float* thr_a0a1);
/* Test hook: the screen32 plan's prune block (64 rows of 20 floats: the fp32
 * centroid, then the direct test's n1, n2 (int32 bits), h3, ec32; then E[64]
 * and h[64]) of centroids C (k, d) from the host plan (which = 0) or the
 * device plan kernel (1), or as the device loop's last finalize left it (2; C
 * unused); out: 1408 floats.                                                 */
int cdr_debug_plan32(cdr_ctx* ctx, int32_t which, const double* C, int32_t k, float* out);
/* Test hook: the plan buffer of the last large-k step, which must have been of
 * k centroids: the fp16 A fragments (KB * DQ * 64 lanes of 16 bytes), the C
 * operand rows (KB * 32 floats), the centroids (k * d doubles), then 16 bytes
 * that begin with the floats {thr1, thr_rel}.  *written = the bytes; out may be
 * null to ask for the size alone.  In a device loop the buffer holds the plan
 * of the loop's current centroids.                                           */
int cdr_debug_big_plan(cdr_ctx* ctx, int32_t k, void* out, int64_t bytes, int64_t* written);

/* ---- per-cluster medians: src/scoring.py:40-55 (np.median) ------------- */
/* Segmented median of float64 values: segment s = values[off[s]..off[s+1]).
 * Empty segment -> NaN; any NaN in a segment -> NaN.                        */
int cdr_medians_segmented(cdr_ctx* ctx, const double* values,
                          const int64_t* offsets, int64_t n_segments,
                          double* out);
/* Array-native form: median of every feature of the local
 * points grouped by the labels of the last Lloyd step; out (k, d).          */
int cdr_medians_by_label(cdr_ctx* ctx, int32_t k, double* out);
/* The same in steps, for points sharded over ranks:
 * cdr_medians_group groups this shard's rows by label (counts[k] = local
 * cluster sizes); after a SUM all-reduce of the counts, cdr_medians_begin
 * takes the global sizes and returns the number of radix passes (4 for F32X
 * points, 8 for F64) and the histogram size in uint32 words (k * d * 512);
 * per pass, cdr_medians_pass_hist writes this shard's digit histograms to
 * `hist` (host or device memory), the caller SUM-all-reduces them, and
 * cdr_medians_pass_select consumes the global histograms; cdr_medians_finish
 * writes out (k, d).  Every rank gets the medians of the whole data set.
 * The grouped rows are valid only for the points, labels and buffers they
 * were built from: loading, generating or restat'ing points, any Lloyd step
 * (it rewrites the labels) and cdr_medians_segmented (it reuses the buffers)
 * discard them, and cdr_medians_begin / _pass_hist / _pass_select / _finish
 * then fail with CDR_ERR_STATE until cdr_medians_group has run again (the
 * pass entries and _finish also until cdr_medians_begin has).               */
int cdr_medians_group(cdr_ctx* ctx, int32_t k, int64_t* counts);
int cdr_medians_begin(cdr_ctx* ctx, const int64_t* global_counts, int32_t* passes,
                      int64_t* hist_words);
int cdr_medians_pass_hist(cdr_ctx* ctx, int32_t pass, void* hist);
int cdr_medians_pass_select(cdr_ctx* ctx, int32_t pass, const void* hist);
int cdr_medians_finish(cdr_ctx* ctx, double* out);

/* ---- medians of all points: src/main.py:31-38 (global_medians) ---------- */
/* out[f] = np.median of feature f over the resident points (the float64
 * conversions of F32X points), exactly what compute_cluster_medians
 * (src/scoring.py:50-54) returns for one cluster holding every file: the
 * scoring's global_medians, which src/main.py:31-38 leaves as placeholders.
 * An MSB radix select over the resident layout itself: no labels, no grouped
 * copy, the histograms stay on the device.  Never -0.0; n = 0 gives NaN.    */
int cdr_medians_global(cdr_ctx* ctx, double* out /* [d] */);
/* The same in steps for points sharded over ranks (src/main.py:31-38,
 * src/scoring.py:50-54): after a SUM all-reduce of the local row counts,
 * cdr_medians_global_begin takes the global count and returns the number of
 * radix passes (4 for F32X points, 8 for F64) and the histogram size in
 * uint32 words (d * 512: [d][2 ranks][256]); per pass,
 * cdr_medians_global_pass_hist writes this shard's digit counts to `hist`
 * (host or device memory), the caller SUM-all-reduces them and
 * cdr_medians_global_pass_select consumes the global counts;
 * cdr_medians_global_finish writes out[d].  The calls keep buffers of their
 * own: labels, grouped rows (cdr_medians_group) and the Lloyd state stay as
 * they are, and a Lloyd step does not disturb them.  Loading, generating or
 * restat'ing points ends the begun state: _pass_hist / _pass_select / _finish
 * then fail with CDR_ERR_STATE until cdr_medians_global_begin has run again.
 * CDR_ERR_STATE without points; CDR_ERR_UNSUPPORTED for 2^32 rows or more
 * (in n_total or in the shard: the counters are uint32).                    */
int cdr_medians_global_begin(cdr_ctx* ctx, int64_t n_total, int32_t* passes,
                             int64_t* hist_words);
int cdr_medians_global_pass_hist(cdr_ctx* ctx, int32_t pass, void* hist);
int cdr_medians_global_pass_select(cdr_ctx* ctx, int32_t pass, const void* hist);
int cdr_medians_global_finish(cdr_ctx* ctx, double* out);
/* out[11] = {histogram kernels ms, the longest of them ms, passes, then the ms
 * of pass 0..7 (0 for passes not run)} of the last cdr_medians_global (HIP events around its launches; src/main.py:31-38,
 * src/scoring.py:50-54 are what it computes).                              */
int cdr_medians_global_timing(cdr_ctx* ctx, double* out);

/* ---- access-log group-by: src/compute_features.py:31-54 ---------------- */
/* Events: file index (row of the manifest, -1 = path not in the manifest),
 * op (1 = WRITE, 2 = READ, other = neither), client id (-1 = null),
 * timestamp in microseconds since the epoch (Spark TimestampType units;
 * INT64_MIN = null: the event counts, the nulls of a file form one more
 * second group, and the max ignores them).
 * primary[f] = client id of file f's primary node (-2 = null).
 * out (n_files, 6) int64: access_freq, writes, reads, local_accesses,
 * total_accesses, max_concurrency (sec = floor(ts_us / 1e6) in fp64, as
 * F.floor(cast(ts as double))).  *max_ts_us = max non-null event timestamp
 * over all events (INT64_MIN when there is none).                          */
int cdr_features_aggregate(cdr_ctx* ctx, int64_t n_events,
                           const int32_t* file_idx, const uint8_t* op,
                           const int32_t* client, const int64_t* ts_us,
                           int64_t n_files, const int32_t* primary,
                           int64_t* out, int64_t* max_ts_us);
/* Config-4 scale runs: a synthetic time-ordered access log generated on
 * the device and kept resident (event e at t0_us + e * span_us / n_events;
 * file uniform over n_files; op WRITE with p = 1/10 else READ; client and
 * primary uniform over 3 datanodes).  cdr_features_aggregate_resident runs
 * the same group-by as cdr_features_aggregate on them (out: host
 * (n_files, 6) or NULL to keep the result on the device);
 * cdr_features_events_read copies the events back (parity tests).          */
int cdr_features_generate(cdr_ctx* ctx, int64_t n_events, int64_t n_files, uint64_t seed,
                          int64_t t0_us, int64_t span_us);
int cdr_features_aggregate_resident(cdr_ctx* ctx, int64_t* out, int64_t* max_ts_us);
/* The reference's access simulator on the device (src/access_simulator.py:
 * 16-60 with src/generator.py:44-45's category weights and primary nodes):
 * files file_begin .. file_begin + n_files - 1 of a manifest, each with a
 * category, jittered read / write rates and locality bias, Poisson arrivals
 * over duration_s seconds from t0_us, timestamps with millisecond precision,
 * clients 0 .. n_clients - 1; the log is left resident sorted by timestamp
 * (file ids local, 0 .. n_files - 1).  *n_events = the events generated.  */
int cdr_features_simulate(cdr_ctx* ctx, int64_t n_files, int64_t file_begin, double duration_s,
                          int32_t n_clients, uint64_t seed, int64_t t0_us, int64_t* n_events);
int cdr_features_events_read(cdr_ctx* ctx, int32_t* file_idx, uint8_t* op, int32_t* client,
                             int64_t* ts_us, int32_t* primary);
/* What the last group-by did: info[0] 1 = hand-written partition + bucket
 * hash path (csrc/groupby.hip), 0 = sort-based path; [1] file-local bits L
 * (2^L files per bucket); [2] partition passes; [3] payload bytes; [4]
 * buckets redone with the global-memory hash; [5] 1 = dense (file, second)
 * grid per bucket, 0 = hash; [6] workgroups of the persistent bucket grid.
 * (info has 7 entries.)                                                    */
int cdr_features_groupby_info(cdr_ctx* ctx, int64_t* info);
/* ---- sharded feature aggregation ------------------ */
/* Rank r owns manifest rows [bounds[r], bounds[r+1]) (nranks + 1 entries,
 * non-decreasing).  cdr_features_exchange_pack: the resident events, grouped
 * by owner rank, as 16-byte records {ts int64, file int32 (global row),
 * client << 8 | op int32} written to `send` (host or device memory, room for
 * every resident event); counts[r] = records for rank r; events outside the
 * manifest are not sent; *max_ts_us = max non-null timestamp over ALL
 * resident events (INT64_MIN if none) for the MAX all-reduce of :48.  The
 * record holds the client as a signed 24-bit value: CDR_ERR_UNSUPPORTED when
 * a record's client is outside [-2^23, 2^23).
 * cdr_features_exchange_unpack: the n records received (host or device
 * memory), all of files [file_begin, file_end), become the resident events
 * with local file ids (and the primaries of those rows move to the front).
 * cdr_features_load_events: host events made resident (the host-tokenised
 * log of a shard).                                                         */
int cdr_features_exchange_pack(cdr_ctx* ctx, int32_t nranks, const int64_t* bounds, void* send,
                               int64_t* counts, int64_t* max_ts_us);
int cdr_features_exchange_unpack(cdr_ctx* ctx, const void* recv, int64_t n, int64_t file_begin,
                                 int64_t file_end);
int cdr_features_load_events(cdr_ctx* ctx, int64_t n, const int32_t* file_idx, const uint8_t* op,
                             const int32_t* client, const int64_t* ts_us, int64_t n_files,
                             const int32_t* primary);
/* Finalisation over sharded rows (:53-94): cdr_features_finalize_stats
 * reduces this rank's n_rows rows to istats[7] = {sum writes, min / max
 * access_freq, min / max writes, min / max concurrency} and dstats[4] = {min /
 * max age, min / max locality} (identities for n_rows == 0); after the SUM /
 * MIN / MAX all-reduce, cdr_features_finalize_apply writes the rows' table
 * with mean(writes) = sum / n_rows_total.  cdr_features_finalize ==
 * stats + apply on one rank.                                               */
int cdr_features_finalize_stats(cdr_ctx* ctx, int64_t n_rows, const int64_t* counts,
                                const double* creation_s, double observation_end,
                                int64_t* istats, double* dstats);
int cdr_features_finalize_apply(cdr_ctx* ctx, int64_t n_rows, const int64_t* counts,
                                const double* creation_s, double observation_end,
                                const int64_t* istats, const double* dstats,
                                int64_t n_rows_total, double* out);
/* Access-log CSV ingest on the device.  Replaces the
 * host read of the log (src/compute_features.py:19-29: spark.read.csv of
 * `ts,path,op,client_node,pid`, to_timestamp; the build's host restatement is
 * compute_features.load_access_log + encode) and the path join against the
 * manifest (:37-41).
 * cdr_ingest_manifest: the manifest's n_files paths (UTF-8 bytes + n_files+1
 *   int64 offsets; an empty string never matches), primary[f] (node id, -2 =
 *   null) and the n_nodes node names whose ids primary uses (bytes + offsets).
 *   Builds device hash tables; CDR_ERR_UNSUPPORTED on a 64-bit hash collision
 *   between distinct strings.
 * cdr_ingest_log: uploads the log bytes and parses them into the resident
 *   events of cdr_features_aggregate_resident (file row or -1, op 1 WRITE /
 *   2 READ / 0, client id or -1 null or -3 not a primary node, ts in
 *   microseconds or INT64_MIN when the timestamp does not parse).
 *   status[6]: records, first bad-timestamp record (-1 none), first record
 *   the device tokeniser does not take (quotes, NUL, lone CR, non-ASCII
 *   timestamp; -1 none), bad-timestamp count, byte span [start, end) from
 *   the end of the previous record to the end of the reported one (blank
 *   lines before it included).  Bad rows are reported in status, not as an error.
 * cdr_ingest_reparse: parses the resident bytes again (benchmarks).        */
int cdr_ingest_manifest(cdr_ctx* ctx, int64_t n_files, const char* path_bytes,
                        const int64_t* path_off, const int32_t* primary, int32_t n_nodes,
                        const char* node_bytes, const int64_t* node_off);
int cdr_ingest_log(cdr_ctx* ctx, const char* bytes, int64_t nbytes, int64_t* status);
int cdr_ingest_reparse(cdr_ctx* ctx, int64_t* status);
/* Finalisation, src/compute_features.py:48-94.  counts: output of
 * cdr_features_aggregate; creation_s: creation_ts_epoch (double seconds, NaN
 * = null -> age 0 as na.fill does); observation_end: max ts in seconds
 * (double).  out (n_files, 10) float64:
 * access_freq, age_seconds, write_ratio, locality, concurrency, then the
 * five *_norm columns.                                                     */
int cdr_features_finalize(cdr_ctx* ctx, int64_t n_files, const int64_t* counts,
                          const double* creation_s, double observation_end,
                          double* out);

/* ---- features CSV on the device: src/compute_features.py:96 ---- */
/* The rows of the features CSV without the header: "path,cell,...,cell\n" per
 * row of table (host, (n_rows, n_cols) row-major), 1 <= n_cols <= 16 (else
 * CDR_ERR_UNSUPPORTED).  Bit j of long_mask prints column j as a long
 * (Python's str(int(v))), the others as the pre-19 JDK's Double.toString
 * (compute_features.java_double_legacy).  The paths are UTF-8 bytes + n_rows+1
 * int64 offsets as in the manifest ingest; a path with ',', '"' or '\n' is wrapped
 * in '"' with every '"' doubled, as csv.writer(lineterminator="\n") does.
 *
 * A row is deferred to the host when a double cell is a subnormal or a finite
 * value outside 2^-128 <= |x| < 2^128, when a long cell is NaN, infinite or
 * |v| >= 2^63, or when its path holds a NUL or CR byte.  It adds no bytes to
 * out and is listed in deferred as the pair {row, byte offset in out where its
 * text belongs}, in row order.  *written = bytes in out, *n_deferred = pairs.
 * CDR_ERR_ARG, with nothing written to out or deferred, when cap or
 * deferred_cap is below what the call needs (the bound below, and n_rows,
 * always suffice).  n_rows == 0 writes nothing.  Runs on the context stream.
 *
 * The bound (host only): 2 * path_bytes_total + n_rows * (3 + 27 * n_cols).
 * The timing entry: out[3] = {cell kernel ms, scan + emit kernels ms, copies ms}
 * of the last format call.                                                    */
int cdr_csv_format(cdr_ctx* ctx, int64_t n_rows, int32_t n_cols, uint32_t long_mask,
                   const double* table, const char* path_bytes, const int64_t* path_off,
                   char* out, int64_t cap, int64_t* written, int64_t* deferred,
                   int64_t deferred_cap, int64_t* n_deferred);
int cdr_csv_bound(int64_t n_rows, int32_t n_cols, int64_t path_bytes_total, int64_t* bytes);
int cdr_csv_timing(cdr_ctx* ctx, double* out);

/* ---- features CSV read on the device: src/main.py:75-81 ---- */
/* pd.read_csv(path)[CLUSTERING_FEATURES].values of the reference, into the
 * resident points: the same float64 bits as pandas' default float parser gives
 * (precise_xstrtod, which is not correctly rounded; csrc/csv_parse.h restates
 * it), in two calls with the caller's host patch between them.
 *
 * cdr_csv_read: bytes[0, nbytes) is the whole file, body_off the offset of the
 *   first byte after the header record (the caller parses the header), n_cols
 *   the header's field count (1..32767), sel[d] the distinct file columns of
 *   the d features (1 <= d <= 16, else CDR_ERR_UNSUPPORTED), in feature order.
 *   Replaces the context's points: finds the records as pandas' tokenizer does
 *   ('\n' outside quotes, a '\r' before it dropped, empty lines skipped, a
 *   last line without '\n' kept), splits each and parses the selected cells
 *   into the F64 point layout.  The points are not usable until the finish.
 *   status[0] = rows, status[1] = deferred rows, status[2] = the file offset of
 *   the first byte where a quote is not where pandas' quoting and plain quote
 *   parity agree (an opening quote not at a field start, a closing quote not
 *   followed by ',', '"', '\r', '\n' or the end, a file that ends inside
 *   quotes) or where a line of blanks and tabs starts (pandas skips it); -1 if
 *   none.  With status[2] >= 0 the rows are not pandas' rows: the caller takes
 *   the whole file to the host.
 *   col_kinds[4 j + t]: cells of feature j of kind t (0 int-like of at most 15
 *   digits, 1 float, 2 empty = NaN, 3 deferred) over the rows with the header's
 *   field count and no quote, NUL or lone CR.
 *   A row is deferred when its field count differs from n_cols, when it holds
 *   a '"', a NUL or a '\r' that is not before its '\n', or when a selected cell
 *   is of kind 3 (csrc/csv_parse.h lists what that is; nothing is guessed).
 *   deferred receives min(status[1], deferred_cap) triples {row, byte begin,
 *   byte end} (file offsets, the terminator excluded) in row order.
 * cdr_csv_read_finish: rows[m] with values (m, d) row-major overwrite the
 *   deferred rows with what the host parsed; X_out, when not NULL, receives
 *   the (n, d) row-major float64 matrix; then the point statistics and the
 *   storage mode are taken exactly as cdr_points_load_f64 ends (CDR_ERR_NAN
 *   for a non-finite value; X_out is complete by then).  CDR_ERR_STATE without
 *   a cdr_csv_read before it.
 * cdr_csv_read_timing: out[4] = {upload, record index, parse kernel, finish}
 *   ms of the last read.                                                     */
int cdr_csv_read(cdr_ctx* ctx, const char* bytes, int64_t nbytes, int64_t body_off,
                 int32_t n_cols, const int32_t* sel, int32_t d, int64_t* status,
                 int64_t* col_kinds, int64_t* deferred, int64_t deferred_cap);
int cdr_csv_read_finish(cdr_ctx* ctx, const int64_t* rows, const double* values, int64_t m,
                        double* X_out);
int cdr_csv_read_timing(cdr_ctx* ctx, double* out);

/* ---- the per-file replication plan (extension: src/main.py:92 forms the ---- */
/* ---- cluster column and drops it) ---------------------------------------- */
/* One text row "path,cluster,category,replication\n" per record of the features
 * CSV, without the header row, in record order (row i belongs to label i, the
 * alignment cdr_csv_read gives the points).
 *
 * cdr_plan_format: bytes[0, nbytes) is the whole file, body_off the offset of
 *   the first byte after the header record, n_cols the header's field count
 *   (1..32767, else CDR_ERR_UNSUPPORTED), path_col the path's column.  labels:
 *   n_labels host values in [0, k), or NULL for the labels of the last
 *   assignment resident in the context (n_labels is then ignored); 1 <= k <=
 *   1024 (else CDR_ERR_UNSUPPORTED).  tails: k slots of 64 bytes, slot j holding
 *   the tail_len[j] <= 63 bytes ",<category>,<factor>\n" of cluster j as the
 *   caller's csv.writer wrote them (the device never quotes).
 *   The records are found exactly as cdr_csv_read finds them.  A row's text is
 *   its path_col field as it stands in the file, ',', the decimal label and
 *   the tail.  The call formats the records [row_begin, row_begin + row_count)
 *   (clipped to the file's): a call with row_begin == 0 uploads the file and
 *   builds the record index, which stays on the device for the following calls
 *   with row_begin > 0 and the same file, k and kind of labels (CDR_ERR_STATE
 *   without it; cdr_csv_read and a failed call drop it).  Resident labels are
 *   checked again on every call.  Device scratch beyond
 *   the file and its index is bounded by row_count; the text does not depend on
 *   the split.
 *   A row is deferred when it holds a '"', a NUL or a '\r' that is not before
 *   its '\n', when its field count differs from n_cols, or when its path field
 *   is longer than 65535 bytes.  It adds no bytes to out and is listed in
 *   deferred as {row, byte offset in out where its text belongs, byte begin,
 *   byte end} (the row of the file; file offsets, the terminator excluded), in
 *   row order; deferred receives min(status[2], deferred_cap) entries.
 *   status[0] = rows of the file, status[1] = bytes in out, status[2] = deferred
 *   rows of this call, status[3] = cdr_csv_read's status[2] (the guard) over the
 *   rows formatted since row_begin == 0, -1 if none: with it >= 0 the rows are
 *   not pandas' rows and the caller takes the whole file to the host.
 *   CDR_ERR_ARG, with nothing written to out or deferred, for a label outside
 *   [0, k), a label count (the context's row count for resident labels) other
 *   than the file's row count, k below the resident labels' k, a tail longer
 *   than 63 bytes, or cap below what the rows need (the bound always suffices;
 *   status[1] then holds what they need and the index stays for a second call);
 *   CDR_ERR_STATE without labels on the device when labels == NULL.  The
 *   context's points, labels and grouped medians are not touched.
 * cdr_plan_bound (host only): field_bytes + n_rows * (1 + 10 + 63), with
 *   field_bytes an upper bound of the rows' path bytes (the body's size is one).
 * cdr_plan_timing: out[5] = {upload, record index, lengths + scan kernels,
 *   emit kernel, copies back} ms, summed over the calls since row_begin == 0.
 * cdr_plan_size_sums: what the plan costs.  For cluster j of labels (n host
 *   values in [0, k), or NULL: the resident labels, n = the context's rows) and
 *   sizes (n host values >= 0, n < 2^31): out[2 j] = the sum of the sizes' low 32
 *   bits, out[2 j + 1] = the sum of their high 31 bits (neither can overflow;
 *   total = out[2 j] + out[2 j + 1] * 2^32).  sizes == NULL counts the rows:
 *   every size is 1 and nothing is uploaded.  CDR_ERR_ARG for a negative size,
 *   a label out of range, or n other than the context's rows with NULL labels. */
int cdr_plan_format(cdr_ctx* ctx, const char* bytes, int64_t nbytes, int64_t body_off,
                    int32_t n_cols, int32_t path_col, const int64_t* labels, int64_t n_labels,
                    int32_t k, const char* tails, const int32_t* tail_len, int64_t row_begin,
                    int64_t row_count, char* out, int64_t cap, int64_t* status, int64_t* deferred,
                    int64_t deferred_cap);
int cdr_plan_bound(int64_t n_rows, int64_t field_bytes, int64_t* bytes);
int cdr_plan_timing(cdr_ctx* ctx, double* out);
int cdr_plan_size_sums(cdr_ctx* ctx, const int64_t* labels, int64_t n, int32_t k,
                       const int64_t* sizes, uint64_t* out /* [k][2] */);

/* ---- two clusterings of the same rows compared (extension: src/main.py:92 -- */
/* ---- forms the cluster column and drops it, so no two runs can be compared) */
/* The contingency table of two labelings a and b of the same n rows:
 * counts[a][b] = the number of rows i with labels_a[i] == a and labels_b[i] == b,
 * exact integers whatever the order of the adds.
 *
 * cdr_agree_keep: copies the labels of the last assignment device to device
 *   into a buffer the context keeps, with their row count and their k.  The
 *   kept labels survive later Lloyd steps and cdr_points_load_f64; only
 *   another keep replaces them.  CDR_ERR_STATE without labels on the device.
 * cdr_agree_table: labels_a: n host values in [0, ka), or NULL for the labels
 *   of the last assignment resident in the context (n must be the context's
 *   row count and ka >= their k).  labels_b: n host values in [0, kb), or NULL
 *   for the kept labels (n must be the kept row count and kb >= the kept k).
 *   1 <= ka, kb <= 1024, else CDR_ERR_UNSUPPORTED.  sizes: n host values >= 0,
 *   and then for every cell size_sums[a][b][0] = the sum of the sizes' low 32
 *   bits, size_sums[a][b][1] = the sum of their high 31 bits over the cell's
 *   rows (neither can overflow; total = [0] + [1] * 2^32); sizes == NULL: the
 *   counts alone, nothing is uploaded for sizes and size_sums must be NULL.
 *   n == 0 gives zero tables.  Tables of at most cdr_agree_info's cap are
 *   summed per workgroup in LDS, larger ones (up to 2^20 cells) with global
 *   integer atomics; the results are the same.
 *   CDR_ERR_ARG for a label out of range on either side, a negative size, n
 *   other than a NULL side's row count, ka or kb below a NULL side's k, n
 *   outside [0, 2^31), or size_sums without sizes (and the reverse);
 *   CDR_ERR_STATE for a NULL side with nothing resident or kept.  After any
 *   error the context stays usable, and a call changes nothing else in it: the
 *   points, the resident and the kept labels, the grouped medians and the
 *   plan's record index are not touched.
 * cdr_agree_info: out[4] = {form of the last cdr_agree_table (0: LDS, 1:
 *   global, -1: none yet), the LDS form's cell cap without sizes, its cap with
 *   sizes, workgroups of the last launch (0: none, n == 0)}.
 * cdr_agree_timing: out[3] = {uploads and zeroing, kernel, copy back} ms of the
 *   last cdr_agree_table, from HIP events.                                   */
int cdr_agree_keep(cdr_ctx* ctx);
int cdr_agree_table(cdr_ctx* ctx, const int64_t* labels_a, int32_t ka, const int64_t* labels_b,
                    int32_t kb, int64_t n, const int64_t* sizes,
                    uint64_t* counts /* [ka][kb] */, uint64_t* size_sums /* [ka][kb][2] or NULL */);
int cdr_agree_info(cdr_ctx* ctx, int64_t* out);
int cdr_agree_timing(cdr_ctx* ctx, double* out);

/* ---- replica placement (extension: no reference counterpart; the reference -- */
/* ---- stops at a replication factor per category, src/main.py:92) ---------- */
/* Where each file's replicas go, from the client node of every resident event
 * (cdr_features_load_events, _generate, _simulate, cdr_ingest_log, the
 * exchange).  For file f and node j < n_nodes, cnt[f][j] = its events with
 * client == j; total[f] = all its events (a client that is negative or >=
 * n_nodes counts in the total only; events with a file outside [0, n_files)
 * are ignored).  The node order of f: its primary first when 0 <= primary <
 * n_nodes, then the other nodes by descending cnt, ties to the lower id.  The
 * first min(factor, n_nodes) of that order are its nodes, factor =
 * factors[labels[f]].  All results are exact integers in any order of the adds.
 *
 * cdr_place_replicas (extension, no reference counterpart): n_nodes in
 *   [1, 64] and k in [1, 1024], else CDR_ERR_UNSUPPORTED; R in [1, 8].
 *   labels: n_labels host values in [0, k) (n_labels must be the events'
 *   n_files), or NULL for the labels of the last assignment resident in the
 *   context (their row count must be n_files, k >= their k).  factors: k
 *   values in [0, R].  sizes: n_files host values >= 0, or NULL.
 *   nodes_out [n_files][R]: the chosen nodes, then -1.  per_file_out
 *   [n_files][3] (may be NULL) = {total, local_before = cnt[f][primary] (0
 *   without a valid primary), local_after = the sum of cnt over the chosen
 *   nodes}.  counts_out [n_files][n_nodes] (may be NULL) = cnt.  cluster_sums
 *   [k][3] = the per_file columns summed over each cluster's files.  node_sums
 *   [n_nodes][3] = {replicas placed on the node, the sum of their sizes' low
 *   32 bits, of their high 31 bits} (bytes = [1] + [2] * 2^32; zeros without
 *   sizes).
 *   The bucket form reads the partition the group-by left resident
 *   (cdr_features_aggregate_resident), or builds it first when the events
 *   were rewritten since; one wave counts a bucket of 2^L files in LDS.  When
 *   the group-by does not take the shape (or CDR_GROUPBY_SORT=1 keeps it off
 *   the partition), when (4 << L) * n_nodes exceeds
 *   12288 bytes, or with CDR_PLACE_GLOBAL=1 in the environment, the global
 *   form counts into a [n_files][n_nodes + 1] table with integer atomics
 *   (n_files * n_nodes <= 2^30, else CDR_ERR_UNSUPPORTED).  Same results.
 *   CDR_ERR_ARG: a label or factor out of range, a negative size, n_labels
 *   other than n_files, R out of range; CDR_ERR_STATE: no resident events, or
 *   NULL labels with none on the device.  After any error the context stays
 *   usable.  cdr_features_aggregate (host events in one call) overwrites the
 *   event buffers without making its events the resident ones: a placement
 *   after it is CDR_ERR_STATE until a loader (cdr_features_load_events, ...)
 *   makes events resident again.  A successful call leaves the points, the resident and kept
 *   labels, the grouped medians, the plan's record index and the events as
 *   they were.
 * cdr_place_info (extension): out[6] = {form of the last call (0 bucket, 1
 *   global, -1 none), L, buckets, workgroups launched, 1 if the resident
 *   partition was reused (0: built by the call), payload bytes}.
 * cdr_place_timing (extension): out[4] = {partition (0 when reused), uploads
 *   and zeroing, kernels, copies back} ms of the last call, from HIP events. */
int cdr_place_replicas(cdr_ctx* ctx, int32_t n_nodes, const int64_t* labels, int64_t n_labels,
                       int32_t k, const int32_t* factors, int32_t R, const int64_t* sizes,
                       int32_t* nodes_out, int64_t* per_file_out, int64_t* counts_out,
                       uint64_t* cluster_sums /* [k][3] */, uint64_t* node_sums /* [n_nodes][3] */);
int cdr_place_info(cdr_ctx* ctx, int64_t* out);
int cdr_place_timing(cdr_ctx* ctx, double* out);

/* How local a GIVEN placement is under the resident events, and what it costs
 * (the evaluation of a placement the call does not choose: yesterday's, or the
 * block locations a cluster really has).  nodes [n_files][R] holds each file's
 * replica nodes, entries in [-1, n_nodes), -1 = no replica.  Per file f:
 * mask[f] = the set of its entries >= 0 (a node listed twice counts once),
 * first[f] = its first entry >= 0 in row order (-1 without one), copies[f] =
 * the size of the set.  An event (f, op, client) with f in [0, n_files) is
 * local when 0 <= client < n_nodes and client is in mask[f]; events of other
 * files are ignored; a client that is no node is never local.  op 1 = WRITE,
 * 2 = READ (the codes of the event loaders).  All results are exact integer
 * sums in any order of the adds.
 *
 * cdr_place_evaluate (extension, no reference counterpart): n_nodes in [1, 64]
 *   and k in [1, 1024], else CDR_ERR_UNSUPPORTED; R in [1, 8].  labels:
 *   n_labels host values in [0, k) (n_labels must be the events' n_files), or
 *   NULL for the labels of the last assignment resident in the context (their
 *   row count must be n_files, k >= their k).
 *   per_file_out [n_files][2] (may be NULL) = {total, local}.  cluster_sums
 *   [k][6], by labels[f] = {events, local, reads, reads_local, writes,
 *   write_copies = the sum of copies[f] over the WRITE events}.  node_sums
 *   [n_nodes][5], for node j = {issued: events with client == j, local: those
 *   of them that are local, reads_served: the local READs of client j plus the
 *   non-local READs of files with first[f] == j (a READ of a file with no
 *   replica is served by nobody), writes_received: the WRITE events of files
 *   with j in mask[f], replicas: the files with j in mask[f]}.
 *   One pass over the files builds a 16-byte record per file; one persistent
 *   kernel streams ev_file / ev_client / ev_op, gathers the file's record and
 *   adds into per-workgroup LDS tables of uint64, flushed once per workgroup.
 *   With per_file_out the kernel also adds into a uint32 [n_files][2] table;
 *   2^32 or more resident events are CDR_ERR_UNSUPPORTED.
 *   CDR_ERR_ARG: R out of range, a node entry or a label out of range,
 *   n_labels other than n_files; CDR_ERR_STATE: no resident events, the event
 *   buffers hold cdr_features_aggregate's host events, or NULL labels with
 *   none on the device.  After any error the context stays usable.  A
 *   successful call leaves the points, the resident and kept labels, the
 *   grouped medians, the plan's record index, the events and the resident
 *   partition (neither used nor dropped) as they were.
 * cdr_place_evaluate_info (extension): out[3] = {form of the last call (0: the
 *   event kernel without the per-file table, 1: with it, -1 none), workgroups
 *   of the event kernel, events per workgroup and sweep}.
 * cdr_place_evaluate_timing (extension): out[4] = {uploads and zeroing, file
 *   pass, event kernel, copies back} ms of the last call, from HIP events. */
int cdr_place_evaluate(cdr_ctx* ctx, int32_t n_nodes, const int32_t* nodes /* [n_files][R] */,
                       int32_t R, const int64_t* labels, int64_t n_labels, int32_t k,
                       int64_t* per_file_out /* [n_files][2] or NULL */,
                       uint64_t* cluster_sums /* [k][6] */, uint64_t* node_sums /* [n_nodes][5] */);
int cdr_place_evaluate_info(cdr_ctx* ctx, int64_t* out);
int cdr_place_evaluate_timing(cdr_ctx* ctx, double* out);

/* ---- cluster quality (extension: no reference counterpart) ------------- */
/* Validity indices of a clustering of the resident points, for choosing the
 * k the reference fixes (src/main.py --k).  The distance is the reference's
 * np.linalg.norm(x - y) (src/kmeans_plusplus.py:33): sqrt(sum_f (x_f - y_f)^2)
 * in fp64 on the float64 values of the points, in either storage mode.  No
 * floating-point atomics: the same input gives bit-identical output.
 *
 * cdr_quality_silhouette: silhouette of the m local rows idx (NULL: all rows,
 *   m == n) with labels in [0, k) (NULL: the labels of the last assignment).
 *   With c_A the rows of the sample labelled A, for row i of cluster A:
 *   a_i = sum_{j in A, j != i} d(i, j) / (c_A - 1), b_i = min over B != A with
 *   c_B > 0 of sum_{j in B} d(i, j) / c_B, s_i = (b_i - a_i) / max(a_i, b_i)
 *   (0 when a_i = b_i = 0 or c_A == 1).  s (m) in the caller's row order;
 *   cluster_sum[j] = sum of s_i over cluster j, cluster_count[j] = c_j (either
 *   may be NULL).  1 <= d <= 64 and k <= 1024, else CDR_ERR_UNSUPPORTED;
 *   CDR_ERR_ARG for m outside [2, 2^20], a row or label out of range, or a
 *   number of non-empty clusters outside [2, m - 1]; CDR_ERR_STATE without
 *   points, or without labels on the device when labels == NULL.
 * cdr_quality_scatter: the device part of Davies-Bouldin over all n rows:
 *   sums[j] = sum over the rows labelled j of d(x, C_j) for centroids C (k, d),
 *   counts[j] = their number; labels NULL (resident) or n values.  Same
 *   shapes and errors.  (S_j = sums / counts; the k x k part is host work.)
 * cdr_quality_timing: out[4] = kernel times of the last calls {silhouette pair
 *   kernels ms (sum), the longest single pair launch ms, pair launches,
 *   scatter kernels ms}.                                                     */
int cdr_quality_silhouette(cdr_ctx* ctx, const int64_t* idx, int64_t m, const int64_t* labels,
                           int32_t k, double* s, double* cluster_sum, int64_t* cluster_count);
int cdr_quality_scatter(cdr_ctx* ctx, const double* C, int32_t k, const int64_t* labels,
                        double* sums, int64_t* counts);
int cdr_quality_timing(cdr_ctx* ctx, double* out);

/* ---- host helpers (plain C on the host, no device) --------------------- */
/* ((init + v[0]) + v[1]) + ... in fp64, left to right.                      */
double cdr_host_seq_sum(const double* v, int64_t n, double init);

#ifdef __cplusplus
}
#endif
#endif /* CDR_H_ */
