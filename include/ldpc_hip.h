/*
 * ldpc_hip.h -- C ABI of libldpc_hip.so: batched flooding-schedule belief propagation on MI355X.
 *
 * This is the drop-in boundary for the one hot path of quantumgizmos/ldpc that this library
 * replaces: ldpc.BpDecoder.decode (src_python/ldpc/bp_decoder/_bp_decoder.pyx:642-695) ->
 * ldpc::bp::BpDecoder::decode (src_cpp/bp.hpp:159-190) -> bp_decode_parallel (bp.hpp:192-325),
 * applied to a BATCH of independent syndromes.  The reference has no FFI for this path today (its
 * Cython layer includes bp.hpp directly, _bp_decoder.pxd:9-83); these entry points are what a
 * binding for a device decoder would bind, one per reference member it stands in for.
 * INTEGRATION.md shows the Cython/ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 (LDPC_HIP_OK) or a negative ldpc_hip_status;
 *     ldpc_hip_last_error() returns a thread-local message for the last failure.  No exceptions
 *     and no aborts cross this boundary (the reference's decode() is not `except +`,
 *     _bp_decoder.pxd:78).
 *   - the caller owns every buffer it passes; the library owns device memory, streams and events
 *     inside the handle.  Data pointers may be host or device pointers (detected per call).
 *   - a handle is single-consumer, like the reference object (its messages live inside H,
 *     bp.hpp:42-48); distinct handles are independent.  An ldpc_hip_bp handle lives on one GPU; an
 *     ldpc_hip_bp_multi handle (end of this file) shards a batch over several GPUs of the node.
 *   - a handle owns ONE workspace and launches on ONE stream at a time (ldpc_hip_bp_set_stream).  The
 *     *_async entry points only queue work; queue the next call on the same stream, or change the stream
 *     first -- ldpc_hip_bp_set_stream orders the new stream after everything the handle has queued so far.
 */
#ifndef LDPC_HIP_H
#define LDPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LDPC_HIP_OK = 0,
    LDPC_HIP_ERR_INVALID = -1,  /* bad argument (shape, range, NULL) */
    LDPC_HIP_ERR_DEVICE = -2,   /* HIP runtime error (message has hipGetErrorString) */
    LDPC_HIP_ERR_NOMEM = -3,    /* workspace does not fit */
    LDPC_HIP_ERR_UNSUPPORTED = -4
} ldpc_hip_status;

/* ldpc::bp::BpMethod, bp.hpp:23-26 */
#define LDPC_HIP_PRODUCT_SUM 0
#define LDPC_HIP_MINIMUM_SUM 1

/*
 * Decoder description = the arguments of ldpc::bp::BpDecoder::BpDecoder (bp.hpp:77-88) that
 * the parallel schedule uses, with the parity-check matrix as CSR instead of a BpSparse&
 * (Py2BpSparse, _bp_decoder.pyx:9-49, builds that from the same coordinates).
 */
typedef struct {
    int32_t m;                    /* check_count  (bp.hpp:56) */
    int32_t n;                    /* bit_count    (bp.hpp:57) */
    int32_t nnz;                  /* = csr_row_ptr[m] */
    const int32_t *csr_row_ptr;   /* [m+1], host */
    const int32_t *csr_col_idx;   /* [nnz], host, strictly ascending inside each row */
    const double *channel_probs;  /* [n], host: channel_probabilities (bp.hpp:55) */
    int32_t max_iter;             /* maximum_iterations (bp.hpp:58), >= 1 */
    int32_t bp_method;            /* LDPC_HIP_PRODUCT_SUM | LDPC_HIP_MINIMUM_SUM (bp.hpp:59) */
    double ms_scaling_factor;     /* bp.hpp:61; 0.0 selects alpha = 1 - 2^-it (bp.hpp:222-228) */
    int32_t device;               /* HIP device ordinal; -1 = current device */
} ldpc_hip_bp_desc;

typedef struct ldpc_hip_bp ldpc_hip_bp; /* opaque handle */

/* replaces: BpDecoderBase.__cinit__ -> new BpDecoderCpp(...)  (_bp_decoder.pyx:118-132) */
int ldpc_hip_bp_create(const ldpc_hip_bp_desc *desc, ldpc_hip_bp **out);

/* replaces: BpDecoderBase.__dealloc__ (_bp_decoder.pyx:162-165) */
void ldpc_hip_bp_destroy(ldpc_hip_bp *h);

/* replaces: writes to bpd.channel_probabilities by the error_rate / error_channel setters and
 * update_channel_probs (_bp_decoder.pyx:180-223).  Priors log((1-p)/p) (bp.hpp:150-151) are
 * evaluated on the host in double precision and uploaded. */
int ldpc_hip_bp_set_channel(ldpc_hip_bp *h, const double *channel_probs, int32_t n);

/* replaces: the max_iter / bp_method / ms_scaling_factor setters (_bp_decoder.pyx:342-394,487-499) */
int ldpc_hip_bp_set_params(ldpc_hip_bp *h, int32_t max_iter, int32_t bp_method,
                           double ms_scaling_factor);

/* replaces: the schedule / serial_schedule_order setters (_bp_decoder.pyx:415-483).  `schedule` uses
 * ldpc::bp::BpSchedule's values (bp.hpp:28-32): 1 = PARALLEL (flooding, default), 0 = SERIAL, 2 = SERIAL_RELATIVE;
 * `serial_schedule_order` (n entries, or NULL for 0..n-1; bp.hpp:110-124) is the order a serial sweep walks.
 * SERIAL with a fixed order runs the tile-wide serial kernels.  Two variants keep STATE in the reference's decoder object
 * and change the order while decoding (bp.hpp:467-483): SERIAL_RELATIVE re-sorts it at the start of every iteration
 * (std::sort by descending prior, then by descending posterior of the previous iteration -- reproduced swap for swap,
 * since ties make the unstable sort's arrangement observable), the random serial schedule (ldpc_hip_bp_set_random_serial)
 * re-shuffles it (std::shuffle on a std::mt19937).  For these, every row of a call starts from the handle's current state
 * (order, generator) and the call leaves the state of its LAST row: a one-row call is exactly one BpDecoder::decode, a
 * sequence of one-row calls exactly a sequence of decodes on one reference object, and a batch on a fresh handle equals a
 * new reference object per row.  Such calls return after the device has finished (the state comes back to the host).
 * This call (re)sets the state to `serial_schedule_order`. */
int ldpc_hip_bp_set_schedule(ldpc_hip_bp *h, int32_t schedule, const int32_t *serial_schedule_order);
/* replaces: the random_serial_schedule / random_schedule_seed setters (_bp_decoder.pyx:527-579 -> bp.hpp:142-145): with
 * `enable` the serial sweep shuffles the order before every iteration; `seed` re-seeds the generator (0 = from the clock, as
 * rng.hpp:117-123 does).  Takes precedence over SERIAL_RELATIVE, as in bp.hpp:467-469.
 * ldpc_hip_bp_soft_info_decode_batch honours the flag the way soft_info_decode_serial does (bp.hpp:573-577): at the top of every
 * iteration that still runs the order is rearranged by std::shuffle with a NEW std::default_random_engine((int32_t)seed) -- the
 * seed as given, 0 included --; rows and state as described above. */
int ldpc_hip_bp_set_random_serial(ldpc_hip_bp *h, int32_t enable, uint32_t seed);
/* the handle's current serial_schedule_order (n entries): what bpd.serial_schedule_order holds after a decode */
int ldpc_hip_bp_get_schedule_order(ldpc_hip_bp *h, int32_t *order);

/* Launch stream (a hipStream_t) for decode calls; NULL selects the handle's own (non-blocking) stream,
 * LDPC_HIP_STREAM_LEGACY_DEFAULT the device's legacy default stream (hipStream_t 0, which is what
 * e.g. torch.cuda.current_stream().cuda_stream reports when no stream context is active). */
#define LDPC_HIP_STREAM_LEGACY_DEFAULT ((void *)1)
int ldpc_hip_bp_set_stream(ldpc_hip_bp *h, void *hip_stream);

/*
 * replaces: BpDecoder.decode for `batch` syndromes at once (_bp_decoder.pyx:676-695 marshalling +
 * bp.hpp:192-325).  Row b of every array belongs to syndrome b.
 *
 *   syndromes  [batch x m] uint8, C-contiguous       in   (bytes as the reference sees them: any
 *                                                          non-zero byte flips the product-sum sign,
 *                                                          min-sum uses the byte's parity, a byte > 1
 *                                                          can never converge: bp.hpp:213,236,300)
 *   decoding   [batch x n] uint8                      out  bpd.decoding          (bp.hpp:62)
 *   llr        [batch x n] float64, or NULL           out  bpd.log_prob_ratios   (bp.hpp:65)
 *   iterations [batch]     int32,  or NULL            out  bpd.iterations        (bp.hpp:69)
 *   converge   [batch]     uint8,  or NULL            out  bpd.converge          (bp.hpp:71)
 *
 * Per-syndrome early exit is preserved: the outputs of row b are those of the first iteration whose
 * hard decision reproduces syndrome b (bp.hpp:300-308), or of iteration max_iter.
 * Synchronous with respect to the host: returns after the results are in the output buffers.
 * Host buffers (the reference API's own mode: NumPy in, NumPy out): a call of at most a few syndromes on a small code works in a
 * host-mapped block (no copy commands).  ONE syndrome of a small code, product-sum, parallel schedule -- the reference's
 * `for shot: decoder.decode(shot)` -- is served by a RESIDENT workgroup (bp_wave_ps_kernel's team form; csrc/host_onchip.h): the kernel
 * that decoded the last syndrome is still there, tables in LDS, polling a request word in the block; the call writes its syndrome,
 * bumps the word and spins on the served word -- no launch, no completion (BB144: 31 -> 22 us a call, hamming(5): 60 -> 50 us;
 * profiles/r5_single_decode_latency.txt).  The workgroup leaves by itself 100 us after its last request, at
 * once when the handle's parameters or priors change or the handle is destroyed; "RESIDENT" 0 = a launch per call.  A large batch (>= 64 MiB of data in at least three chunks, everything in host memory, BP
 * alone, rows independent of one another: the parallel and the fixed-order serial schedule) is cut into chunks of whole tiles --
 * <= 16 384 rows, ~256 MiB of results -- that move through PINNED double buffers on two copy streams: while the kernels decode
 * chunk c, chunk c + 1 is on its way in, chunk c - 1 on its way out, and the calling thread copies chunk c - 2 from the pinned
 * buffer into the caller's (pageable) arrays; with log-ratios the last quarter of the batch goes in chunks that halve down to 4 096 rows
 * (the last chunk's results cross PCIe with nothing left to overlap them).  Results are those of one undivided call.  Debug switches "NO_HOST_PIPELINE",
 * "HOST_CHUNK_ROWS" (tests, measurements).  Measured (bench.py `host_io`): 0.93 of the device-resident rate without LLRs.
 */
int ldpc_hip_bp_decode_batch(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                             uint8_t *decoding, double *llr, int32_t *iterations,
                             uint8_t *converge);

/* Same, but only enqueues on the launch stream and returns without waiting for the device (no host synchronisation:
 * the number of tiles the streaming kernel hands to the per-pass kernels stays on the device, and the per-pass rounds
 * are queued for all of max_iter -- a host-mapped flag the device sets when nothing is left merely lets the host stop
 * queueing early).  All pointers must be device pointers.  Exceptions: a batch that does not fit the workspace in one
 * piece (> 2 097 152 syndromes, or device memory) waits between pieces; the repacked schedules (ldpc_hip_bp_set_repack)
 * wait where noted there. */
int ldpc_hip_bp_decode_batch_async(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                                   uint8_t *decoding, double *llr, int32_t *iterations,
                                   uint8_t *converge);

/*
 * replaces: BpOsdDecoder.decode with osd_method = OSD_0 for `batch` syndromes
 * (src_python/ldpc/bposd_decoder/_bposd_decoder.pyx:125-134): belief propagation as above, then for every
 * row BP left unconverged ldpc::osd::OsdDecoder::decode with osd_order 0 (src_cpp/osd.hpp:110-117) =
 * soft_decision_col_sort (sort.hpp:48-62; stable, ties by ascending column) + RowReduce::fast_solve
 * (gf2sparse_linalg.hpp:298-401) + lu_solve (:237-288), all on the device.  `decoding` receives the BP
 * decision for converged rows and the OSD-0 solution otherwise; llr / iterations / converge are BP's
 * (bpd.log_prob_ratios, bpd.iterations, bpd.converge), any of them may be NULL.
 * The bit-packed [H | s] of one syndrome must fit in LDS (m * ceil((n+1)/64) * 8 + 13 n + 4 m <= 150 KiB),
 * else LDPC_HIP_ERR_UNSUPPORTED.  Syndromes outside the image of H: see ldpc_hip_bposd_get_status.
 */
int ldpc_hip_bposd0_decode_batch(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                                 uint8_t *decoding, double *llr, int32_t *iterations,
                                 uint8_t *converge);
int ldpc_hip_bposd0_decode_batch_async(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                                       uint8_t *decoding, double *llr, int32_t *iterations,
                                       uint8_t *converge);

/*
 * Row priors: every syndrome decoded with its OWN channel probabilities.
 * replaces: the per-shot loop `dec.update_channel_probs(p[shot]); out[shot] = dec.decode(s[shot])` -- BpDecoderBase.update_channel_probs /
 * the error_channel setter (src_python/ldpc/bp_decoder/_bp_decoder.pyx:205-233) followed by BpDecoder.decode (pyx:642-695), whose
 * BpDecoder::initialise_log_domain_bp re-reads channel_probabilities on every decode (src_cpp/bp.hpp:147-157) -- as ONE batch; the
 * bposd0 forms replace the same loop around BpOsdDecoder.decode with osd_method = OSD_0 (_bposd_decoder.pyx:125-134; osd.hpp:110-117
 * orders the columns by BP's posteriors and reads no prior).  The reference's own analog memory experiment runs this loop
 * (monte_carlo_simulation/memory_experiment_v2.py:55-58, 103-113).
 * channel_probs [batch][n]: row b is what the reference would have been given before decoding syndrome b; log((1 - p) / p) is formed on the
 * device with a correctly rounded division and the bit-exact twin of the host's log (bp.hpp:150-151), so p = 0, 1, 0.5 give the
 * reference's +inf, -inf, +0.0 priors.  Outputs as for ldpc_hip_bp_decode_batch / ldpc_hip_bposd0_decode_batch, row for row what that
 * loop returns.  UNLIKE the loop, the handle's own channel probabilities are untouched: the next plain decode uses them as before.
 * Host or device pointers as for the syndromes (each pointer on its own); a host array of probabilities is checked (a value outside
 * [0, 1] or NaN: LDPC_HIP_ERR_INVALID), a device array is the caller's word.  The *_async forms take device pointers only and do not wait.
 * Parallel schedule only: any serial schedule -> LDPC_HIP_ERR_UNSUPPORTED (ldpc_hip_last_error says so).  Higher-order OSD weighs its
 * candidates by log(1 / p) (osd.hpp:134) and has no such form.  Kernels: codes that stream run the per-pass kernels from the first
 * iteration with a per-lane prior; min-sum on a code the lane = edge kernels take (ldpc_hip_bp_set_small_code_kernel: rows <= 4 and
 * columns <= 2 with m <= 256, or rows <= 8 and columns <= 4 with 8 m <= 768; modes -1, 1, 6) runs their row-prior forms
 * (csrc/bp_edge_rp_kernel.h), a wavefront reading its syndrome's priors from a row-major array of log-ratios; every other code an
 * on-chip kernel takes runs the slot kernel (csrc/bp_small_kernel.h), each slot holding its syndrome's priors.  Extra workspace:
 * 512 n bytes per 64-syndrome tile (8 n bytes per syndrome on the lane = edge kernels).
 */
int ldpc_hip_bp_decode_batch_priors(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch, uint8_t *decoding, double *llr,
                                    int32_t *iterations, uint8_t *converge, const double *channel_probs);
int ldpc_hip_bp_decode_batch_priors_async(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch, uint8_t *decoding, double *llr,
                                          int32_t *iterations, uint8_t *converge, const double *channel_probs);
int ldpc_hip_bposd0_decode_batch_priors(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch, uint8_t *decoding, double *llr,
                                        int32_t *iterations, uint8_t *converge, const double *channel_probs);
int ldpc_hip_bposd0_decode_batch_priors_async(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch, uint8_t *decoding, double *llr,
                                              int32_t *iterations, uint8_t *converge, const double *channel_probs);

/*
 * BP + ordered-statistics decoding of any order: replaces BpOsdDecoder.decode's per-shot path for
 * osd_method OSD_E / OSD_CS as well (ldpc::osd::OsdDecoder::decode, src_cpp/osd.hpp:103-187; candidate strings
 * osd.hpp:75-101).  ldpc_hip_bp_set_osd stores the method and order the BpOsdDecoder setters write
 * (_bposd_decoder.pyx:161-234): osd_method 0 = OSD_OFF, 1 = OSD_0, 2 = OSD_E (exhaustive), 3 = OSD_CS
 * (combination sweep) -- the values of ldpc::osd::OsdMethod (osd.hpp:18-23); osd_order >= 0, 0 with OSD_0.
 * ldpc_hip_bposd_decode_batch then post-processes every row BP left unconverged: column sort by log-ratio,
 * reduced row echelon form over that order, the OSD-0 solution, and the sweep over the candidate strings on the
 * non-pivot columns; a candidate replaces the current solution only if its weight sum_j x_j log(1 / p_j)
 * (added up in ascending j, as osd.hpp:171-176 does) is STRICTLY smaller.  osd_order == 0 takes the OSD-0
 * branch whatever the method (osd.hpp:114).  Outputs as for ldpc_hip_bposd0_decode_batch.
 * Limits: the LDS bound of OSD-0 (plus 8 m + 4 n bytes); OSD_E osd_order <= 24 (2^24 candidates per syndrome; the reference
 * itself keeps 2^order strings of k bytes in memory and warns above 15), else LDPC_HIP_ERR_UNSUPPORTED.  OSD_CS takes any
 * osd_order: the k weight-one strings, then the pairs (i, j), i < j < osd_order, among ALL k = n - rank non-pivot columns
 * (pairs whose second index reaches past k are skipped -- the reference writes past its candidate string there, osd.hpp:92-96,
 * undefined behaviour).  Syndromes outside the image of H: see below.
 */
int ldpc_hip_bp_set_osd(ldpc_hip_bp *h, int32_t osd_method, int32_t osd_order);
/*
 * Syndromes outside the image of H.  Every H e is inside; a rank-deficient H (toric-code checks, any H with dependent
 * rows) fed with a syndrome that breaks a dependency is not, and then NO x satisfies H x = s.  The reference still
 * returns a vector: RowReduce::fast_solve never reaches its early stop, eliminates every column, and lu_solve
 * (gf2sparse_linalg.hpp:237-288) solves the equations of the PIVOT ROWS only -- which rows those are is decided by the
 * sparsity heuristic of its linked-list elimination (fewest entries across L and U, ties by the position in the pivot
 * column's linked list, :149-163 / :318-333 -- a position that swap_rows, insert_entry and add_rows leave history-dependent).
 * The bit-packed device eliminations take the first candidate row, which for a syndrome inside the image cannot change the
 * solution.  Rows outside the image are detected (H x != s after the first pass) and go through a second pass: one workgroup
 * per such row re-enacts the reference's elimination on that data structure (csrc/osd_exact_kernel.h) to learn ITS pivot
 * rows, writes the syndrome that agrees with s on those rows and lies in the image, and the same OSD kernels run again on it
 * -- OSD-0, OSD_E and OSD_CS alike.  The output is then the reference's vector, bit for bit (tests/golden/outimage_*.npz,
 * every row), and the row stays flagged: after any ldpc_hip_bposd*_decode_batch call, ldpc_hip_bposd_get_status fills
 * status[batch] (host or device pointer) with
 *   0  BP converged, OSD did not run            1  OSD ran and H x = s
 *   2  OSD ran, s is outside the image of H: x does not (cannot) satisfy H x = s; it solves the reference's pivot rows.
 * `batch` must be the batch size of that decode.  The second pass needs rank H (worked out on the host for m * m * n / 64 < 4e9)
 * and m <= 8192; beyond that a flagged row keeps the solution of the device's own pivot rows.  Both extra launches size
 * themselves from device-side counters: no host round trip, a few microseconds when no row is flagged, nothing at all for
 * a full-rank H.  Device memory of the second pass (per handle, allocated on the first BP + OSD call on a rank-deficient H and
 * kept): the working copies of at most 64 workgroups, (m * ceil(n / 64) + n * m / 4) 64-bit words each, capped at 256 MiB in
 * total, plus batch * (m + 4) bytes for the corrected syndromes and their list; the first such call also pays the host
 * elimination that finds rank H.  If that memory cannot be had the pass is skipped: the decode still succeeds and flagged rows
 * keep the device's own pivot-row solution (status 2).
 */
int ldpc_hip_bposd_get_status(ldpc_hip_bp *h, uint8_t *status, int64_t batch);
/* Serial schedule: a 64-syndrome tile is decoded by one wavefront, which runs until its slowest syndrome is done.  With
 * repacking a first pass of `first_pass_iters` iterations runs over the whole batch and the rows it leaves unconverged are
 * packed into dense tiles and decoded again from the start with the full max_iter (deterministic: same results).
 * -1 = automatic (max_iter / 8, default), 0 = off.  With repacking the call waits once for the device.
 * The STREAMED serial kernels (ldpc_hip_bp_set_serial_kernel: (3,6)-regular-shaped matrices beyond LDS, e.g. the n = 10 000 code)
 * decode in PASSES and never start again: the first pass ends after first_pass_iters iterations (-1 = automatic: 4), the next after
 * twice as many -- or, when a pass left less than 40 % of its rows, after one more iteration.  After a pass the rows still decoding
 * are counted (the call waits for the device once per pass) and either carry on in their tiles (most rows left), or have their
 * message state compacted, lane by lane, into dense tiles, or -- 2048 rows and fewer -- finish a workgroup per syndrome
 * (bp_serial_lane_kernel: the one hopeless syndrome of a batch costs milliseconds instead of keeping a 64-syndrome tile on one
 * compute unit for max_iter iterations).  0 = one pass.  Same results whatever the passes (tests/test_gpu_serial_stream.py).
 * The streamed parallel schedule (codes too large for the on-chip kernels, batches of >= 32768 syndromes) cuts a decode in two
 * as well, but CARRIES ON instead of starting again: after the first pass the message state of the unconverged rows is
 * gathered, lane by lane, out of the first pass's 64-syndrome tiles into dense tiles and the second pass continues from
 * iteration first_pass_iters + 1 (a tile moves all 64 lanes' messages until its slowest syndrome is done; after the
 * compaction the tiles hold live lanes only).  There "automatic" prices a cut at every iteration against the plain run with
 * the iteration histogram the previous decode on the handle left behind, and runs plain when that says so or says nothing
 * yet -- no work is wasted where nothing converges.  Nothing of this waits for the device (the *_async entry points stay
 * asynchronous): the histogram is used only once its copy is SEEN to have landed (a look at an event, never a wait -- decodes
 * queued back to back are steered by the last one that did land), and the second pass is queued at once for the most rows
 * there can be: the device lists the unconverged rows, counts them, and every kernel of the second pass reads that count and
 * reaches the caller's arrays through the list (no rows are copied out and back; no extra message memory: the compacted state
 * is gathered into the first pass's check_to_bit array, which is dead by then).  A batch that does not fit in one chunk of
 * device memory runs plain.
 * The float32 message mode (ldpc_hip_bp_set_message_dtype) is steered by the same setting in the same way on its per-pass route
 * (codes its on-chip kernels do not take): -1 = the last landed histogram decides (default), 0 = off, k = a first pass of k
 * iterations; it applies for 2 <= k < max_iter, max_iter >= 8, batches of >= 32768 syndromes that fit one chunk, and gives every
 * row the bits of the plain float32 decode.  The handle keeps ONE histogram: one left by a float64 decode may steer a float32
 * decode and the other way round (results do not depend on it). */
int ldpc_hip_bp_set_repack(ldpc_hip_bp *h, int32_t first_pass_iters);
/* Serial schedule kernels: bits that share no check commute, so the schedule is cut into levels of mutually check-disjoint
 * bits (level = 1 + the highest level among the EARLIER bits sharing a check) and a workgroup runs a tile level by level
 * with its wavefronts sharing each level's bits -- same results as the bit-by-bit walk.  -1 = automatic (level-parallel
 * when a level holds >= 2 bits on average; STREAMED -- below -- where the matrix allows it and a level holds >= 32 bits),
 * 0 = one wavefront walks the tile bit by bit, 1 = always level-parallel (never streamed), 2 = streamed whenever the matrix allows
 * it.  Streamed (csrc/bp_serial_stream_kernel.h; matrices with one row weight 6 and one column weight 3): the level-parallel
 * form with the message traffic of the flooding kernel -- one record per position of the level-major order (the 15 segments to
 * fetch, the 3 to write, the bit) read through the scalar cache two steps ahead, the segments of the next position in flight into
 * a per-wavefront LDS ring (buffer_load ... lds, counted waits), no initial messages in memory (entries nobody has written yet
 * are the same in all lanes: a per-position table), a decode in passes (ldpc_hip_bp_set_repack) and, for a handful of syndromes
 * (what a pass leaves, or a batch of <= 256), a workgroup per syndrome with the level's bits across the lanes.  The n = 10 000
 * code at p = 0.05, B = 65 536: 171 k -> 692 k syndromes/s; its first pass moves 5.1 TB/s (profiles/r5_serial_stream_summary.txt). */
int ldpc_hip_bp_set_serial_kernel(ldpc_hip_bp *h, int32_t mode);
/* Where the elimination keeps [H | s]: -1 = automatic (in the wavefront's registers when m <= 256 and n <= 511, else
 * one wavefront per syndrome with [H | s] bit-packed in LDS while four of them fit a CU, else one workgroup per syndrome
 * with H in LDS or, beyond 150 KiB, in an HBM scratch slot -- as long as the column order and, for OSD_E / OSD_CS, the
 * candidate tables fit LDS: OSD-0 n <= ~14 000; otherwise LDPC_HIP_ERR_UNSUPPORTED), 0 = the one-wavefront LDS kernels
 * while they fit at all, 2 = a workgroup per syndrome with H in HBM whatever the size.  Results are identical. */
int ldpc_hip_bp_set_osd_kernel(ldpc_hip_bp *h, int32_t mode);
int ldpc_hip_bposd_decode_batch(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                                uint8_t *decoding, double *llr, int32_t *iterations,
                                uint8_t *converge);
int ldpc_hip_bposd_decode_batch_async(ldpc_hip_bp *h, const uint8_t *syndromes, int64_t batch,
                                      uint8_t *decoding, double *llr, int32_t *iterations,
                                      uint8_t *converge);

/*
 * replaces: ldpc::bp::BpDecoder::soft_info_decode_serial (src_cpp/bp.hpp:547-660), the method behind
 * SoftInfoBpDecoder.decode (_bp_decoder.pyx:712-785), over a batch of analog syndromes.
 * soft_syndromes [batch][m] FP64 readouts; each is scaled to 2 s / sigma^2, its sign gives the hard syndrome, and the
 * serial minimum-sum sweep treats a check whose scaled magnitude is below `cutoff` (and below the smallest incoming
 * message) as a virtual variable node that may be updated or flipped (bp.hpp:597-621).  Uses the handle's
 * max_iter, ms_scaling_factor (taken literally, no adaptive mode), channel probabilities and -- if one was set with
 * ldpc_hip_bp_set_schedule(serial, order) -- serial_schedule_order; bp_method and schedule are ignored (the reference
 * class forces minimum_sum / serial, pyx:751-752).  Outputs: decoding [batch][n]; llr, iterations, converge as for
 * decode_batch; soft_syndromes_out [batch][m] = the decoder's soft_syndrome member afterwards (pyx:787-798).  Any
 * output but decoding may be NULL.  Host or device pointers.  m <= 19200 (one word per check in LDS).
 */
int ldpc_hip_bp_soft_info_decode_batch(ldpc_hip_bp *h, const double *soft_syndromes, int64_t batch, double cutoff,
                                       double sigma, uint8_t *decoding, double *llr, int32_t *iterations,
                                       uint8_t *converge, double *soft_syndromes_out);

/*
 * Bit-packed shot data in, bit-packed predictions out: replaces the per-shot loop of the reference's sinter decoders
 * (sinter_decoders/sinter_bposd_decoder.py:115-130, sinter_belief_find_decoder.py; `decode_via_files` reads detection
 * events and writes observable predictions in stim's "b8" format: bit i of a shot is bit i % 8 of its byte i / 8, every
 * shot starts on a byte boundary).
 * ldpc_hip_bp_set_observables uploads the k x n observables matrix L (CSR, as `matrices.observables_matrix`).
 * ldpc_hip_bp_decode_b8: dets_b8 [batch][ceil(m/8)] -> decode every shot (BP; with_osd != 0: BP + the handle's OSD
 * method, see ldpc_hip_bp_set_osd) -> obs_b8 [batch][ceil(k/8)] = L x mod 2 (`(observables_matrix @ corr) % 2`) and/or
 * decoding_b8 [batch][ceil(n/8)] = x.  Either output may be NULL; iterations / converge as for decode_batch (NULL
 * allowed).  All-zero shots yield the zero correction, converge 1, iterations 0 (the Python-level shortcut,
 * _bposd_decoder.pyx:118-123).  Host or device pointers.
 */
int ldpc_hip_bp_set_observables(ldpc_hip_bp *h, int32_t k, const int32_t *csr_row_ptr, const int32_t *csr_col_idx);
/* [batch][bits] one byte per bit <-> [batch][ceil(bits/8)] b8 rows, device pointers only, queued on the handle's
 * stream without synchronisation.  For packing decodings before they cross a link (the multi-GPU gather of
 * bench.py / ldpc_amd.sharding sends 1/8 of the bytes this way). */
int ldpc_hip_pack_b8(ldpc_hip_bp *h, const uint8_t *bytes, int64_t batch, int32_t bits, uint8_t *packed);
int ldpc_hip_unpack_b8(ldpc_hip_bp *h, const uint8_t *packed, int64_t batch, int32_t bits, uint8_t *bytes);
int ldpc_hip_bp_decode_b8(ldpc_hip_bp *h, const uint8_t *dets_b8, int64_t batch, int32_t with_osd, uint8_t *obs_b8,
                          uint8_t *decoding_b8, int32_t *iterations, uint8_t *converge);

/*
 * replaces: GF2Sparse::mulvec (gf2sparse.hpp:177-214) over a batch:
 * out[b][i] = XOR_{j in row i} in[b][j].  Used by received-vector mode (bp.hpp:162-180).
 */
int ldpc_hip_gf2_mulvec_batch(ldpc_hip_bp *h, const uint8_t *vectors, int64_t batch,
                              uint8_t *out_syndromes);

/*
 * Synthetic input generator for benchmarks: independent BSC errors
 * e[b][j] = ((splitmix64(seed, (shot0+b)*n + j) >> 11) < threshold)  (noise model of
 * noise_models/bsc.py:4-23 with a counter-based stream) and syndromes = H e mod 2
 * (mcs.py:124-126).  `errors` may be NULL.  Device or host output pointers.
 */
int ldpc_hip_gen_bsc_syndromes(ldpc_hip_bp *h, uint64_t seed, uint64_t threshold, int64_t shot0,
                               int64_t batch, uint8_t *syndromes, uint8_t *errors);

/*
 * Sampling a detector error model on the device, and the loop around it: a logical error count for (H, L, p) with nothing but two
 * counters crossing the link.  No reference counterpart (stim's compile_sampler plays that role for the reference's users): the
 * specification is the NumPy twin ldpc_amd.noise_models.generate_dem_batch, reproduced bit for bit.
 *   T[j]     = min(max(ceil(p[j] * 2^53), 0), 2^53)                         (float64 on the host; exact)
 *   e[b][j]  = ((splitmix64(seed, (shot0 + b) * n + j) >> 11) < T[j])        (index in uint64: the convention of ldpc_hip_gen_bsc_syndromes,
 *                                                                            whose errors these are when all p[j] are equal)
 *   dets[b]  = H e[b] mod 2,  obs[b] = L e[b] mod 2                         (b8 rows as for ldpc_hip_bp_decode_b8, padding bits 0)
 * ldpc_hip_bp_set_sampler: the per-column probabilities (NULL: the handle's channel probabilities as they are now), checked (outside
 *   [0, 1] or NaN: LDPC_HIP_ERR_INVALID) and uploaded as thresholds.  Independent of the decoding priors: later ldpc_hip_bp_set_channel calls
 *   do not change what is sampled.  L is the matrix of ldpc_hip_bp_set_observables, set before or after.
 * ldpc_hip_bp_sample_b8: shots shot0 .. shot0 + batch - 1 of stream `seed`: dets_b8 [batch][ceil(m/8)], obs_b8 [batch][ceil(k/8)] (NULL
 *   allowed), errors_b8 [batch][ceil(n/8)] (NULL allowed).  Device or host pointers.  No sampler set, obs_b8 without observables, negative
 *   shot0 / batch: LDPC_HIP_ERR_INVALID; batch 0: LDPC_HIP_OK.  A shot's detectors and observables are accumulated in LDS:
 *   ceil(m / 32) + ceil(k / 32) > 4096 words (k counted when obs_b8 is asked for) is LDPC_HIP_ERR_UNSUPPORTED, before anything is launched.
 * ldpc_hip_count_mismatch_b8: *count = rows in which a_b8 and b_b8 ([batch][ceil(bits/8)]) differ in their first `bits` bits (padding is
 *   ignored); row_flags [batch] (NULL allowed) = 1 for those rows.  Device or host pointers, each on its own.
 * ldpc_hip_bp_simulate_b8: shots shot0 .. shot0 + shots - 1 in chunks of `chunk` (<= 0: the library chooses), per chunk on the handle's stream:
 *   sample, decode as ldpc_hip_bp_decode_b8 does (with_osd as there; same refusals in the float32 message mode), predict observables, count.
 *   out[0] = shots whose predicted observables differ from the true ones, out[1] = rows BP left unconverged (converge 0 of decode_b8).
 *   Neither depends on `chunk`.  Needs a sampler and observables (else LDPC_HIP_ERR_INVALID).
 */
int ldpc_hip_bp_set_sampler(ldpc_hip_bp *h, const double *probs);
int ldpc_hip_bp_sample_b8(ldpc_hip_bp *h, uint64_t seed, int64_t shot0, int64_t batch, uint8_t *dets_b8, uint8_t *obs_b8,
                          uint8_t *errors_b8);
int ldpc_hip_count_mismatch_b8(ldpc_hip_bp *h, const uint8_t *a_b8, const uint8_t *b_b8, int64_t batch, int32_t bits, uint64_t *count,
                               uint8_t *row_flags);
int ldpc_hip_bp_simulate_b8(ldpc_hip_bp *h, uint64_t seed, int64_t shot0, int64_t shots, int64_t chunk, int32_t with_osd, uint64_t *out);

/* Duration in milliseconds of the BP kernel launch of the last decode call on this handle,
 * measured with HIP events on the launch stream (0 if none yet).  Also 0 after a call of at most four syndromes with host buffers
 * on a small code (a single decode()): there the two event packets would cost more than they tell -- debug switch
 * "TIME_SMALL_CALLS" = 1 keeps them.  After a large call with host buffers (pinned chunks, see ldpc_hip_bp_decode_batch) it
 * describes the LAST chunk only. */
int ldpc_hip_bp_last_kernel_ms(ldpc_hip_bp *h, float *ms);
/* Split of that time for the streaming path: the persistent kernel (bp_decode_kernel) and the per-pass launches
 * (bp_spread_*_kernel: small batches from the first iteration, stragglers of large ones).  Both 0 for other kernels. */
int ldpc_hip_bp_last_phase_ms(ldpc_hip_bp *h, float *persistent_ms, float *per_pass_ms);

/* Bytes of device workspace a decode of `batch` syndromes needs (message arrays dominate:
 * 2 * 8 * nnz bytes per syndrome; 2 * 4 * nnz with LDPC_HIP_MSG_F32). */
int64_t ldpc_hip_bp_workspace_bytes(const ldpc_hip_bp *h, int64_t batch);

/* Tuning knobs (0 = library default): wavefronts per workgroup of the BP kernel (1..16) and the
 * largest number of 64-syndrome tiles decoded per launch (bounds the workspace). */
int ldpc_hip_bp_set_tuning(ldpc_hip_bp *h, int32_t waves_per_workgroup, int32_t max_chunk_tiles);

/*
 * How the product-sum update evaluates std::tanh / std::log of bp.hpp:208-217 on the device:
 *   LDPC_HIP_MATH_LIBM_EXACT (default): re-implementations of the host glibc's tanh (fdlibm expm1
 *       based) and log (table driven, FMA build) that are bit-identical to them, so log_prob_ratios
 *       equal the reference's to the last bit (as min-sum's always do);
 *   LDPC_HIP_MATH_FAST: ~1-ulp routines, ~40 % fewer FP64 operations; hard decisions identical
 *       except on exact ties of the reference's posterior, LLRs within the 1e-5 relative tolerance.
 */
/* For matrices whose rows all have one weight and whose columns all have one weight the BP kernel
 * streams messages through a per-wavefront LDS ring filled by asynchronous global->LDS loads
 * (default: 2 slots per wavefront).  depth 0 forces the register-prefetch variant used for irregular
 * matrices, 2 or 3 select the ring depth (1 = default); results are identical in every case.  (Irregular matrices with rows of
 * <= 16 and columns of <= 8 entries have a ring of their own -- a queue of 1 KiB units, debug switch "VAR_RING" 1 -- which is built and
 * tested but not selected by default: see ldpc_hip_bp_set_handoff.) */
int ldpc_hip_bp_set_ring(ldpc_hip_bp *h, int32_t depth);

/* Straggler hand-off of the streaming BP kernel.  A 64-syndrome tile is decoded by one persistent workgroup,
 * i.e. on one compute unit; when no more than `threshold_tiles` tiles are still running (a few syndromes that
 * refuse to converge, a tiny batch, or the reference's default max_iter = n) those tiles park their state and
 * their remaining iterations run as per-pass launches (check pass, bit pass, syndrome test, bookkeeping) spread
 * over the whole chip; a batch of no more than `threshold_tiles` tiles runs that way from the first iteration.
 * -1 = automatic (default): 256 tiles -- except for product-sum on a matrix that has no fixed-degree ring variant (irregular codes; rows <= 16,
 * columns <= 8 entries), where every batch runs as per-pass launches from its first iteration (the persistent kernel's single register
 * allocation leaves three wavefronts per SIMD there, the per-pass kernels run 4 - 8: 0.45 -> 0.56 of HBM on the irregular n = 10 000 code);
 * 0 = off; any value set here is taken as given.  Results are identical.  The hand-off costs no host synchronisation. */
int ldpc_hip_bp_set_handoff(ldpc_hip_bp *h, int32_t threshold_tiles);

/* Codes whose two message arrays fit in a few KiB per syndrome (surface codes, bivariate-bicycle codes)
 * are decoded by on-chip kernels: messages live in LDS and a syndrome that converges is replaced at once.
 * Two variants: one wavefront per syndrome with no workgroup barrier in the loop (row and column weights <= 8),
 * and a workgroup that keeps up to four syndromes resident (any degrees).  mode -1 = automatic (default),
 * 0 = always use the streaming kernel, 1 = use an on-chip kernel whenever one syndrome fits in LDS,
 * 2 = as 1 but only the workgroup ("slot") variant, 3 = as 1 but only the lane = node wavefront variant (product-sum
 * otherwise prefers a lane = entry variant that keeps every lane busy with one transcendental).  That variant gives a syndrome
 * one wavefront, or -- where LDS leaves room for fewer than six syndromes per compute unit, e.g. a 768 x 1600 matrix -- all the
 * wavefronts of a workgroup (its "team" form); 4 = as 3, one wavefront per syndrome, 5 = as 3, a workgroup per syndrome.
 * Min-sum on matrices with rows of weight <= 4 and columns of weight 1 .. 2 (rotated / toric surface codes, ring codes; m <= 256)
 * takes a third variant in modes -1, 1 and 6: lane = EDGE, a row's entries in four neighbouring lanes, every message in a
 * register for the whole decode (bp_edge_kernel.h: bp_edge_kernel); with rows of weight <= 8 and columns of weight <= 4
 * (8 m <= 768: the bivariate-bicycle family) the same idea with a row in EIGHT neighbouring lanes (bp_edge8_kernel).
 * 6 = those variants where they apply, else as -1.  The on-chip kernels take batches below 2^30 syndromes (larger ones
 * are streamed).  Results are identical.
 * Row priors (ldpc_hip_*_decode_batch_priors): mode 0 = the per-pass kernels; modes -1, 1, 6 with min-sum on a code of the lane = edge
 * variants = their row-prior forms (bp_edge_rp_kernel, bp_edge8_rp_kernel); modes 3, 4, 5 with min-sum on a code the lane = node variant
 * takes (rows <= 16, columns <= 8, a syndrome's state within LDS) = its row-prior form (bp_wave_rp_kernel: 3 its own choice between one
 * wavefront and a team per syndrome, 4 / 5 force either) -- modes -1, 1, 6 take it for such a code beyond the lane = edge variants too
 * (the debug switch "WAVE_RP" 0 switches that off); any other code an on-chip kernel would take, and mode 2 always = the
 * slot variant, which reads a prior per syndrome too, if one slot fits 150 KiB of LDS, else the per-pass kernels.  All routes give the same bits.
 *   ldpc_hip_bp_row_prior_route(h, batch, want_llr, &route): which kernels a row-prior decode of `batch` syndromes takes on this handle as it is
 *       set now, whether or not priors are staged -- 0 the per-pass kernels, 1 bp_edge, 2 bp_edge8, 3 bp_wave with one wavefront per syndrome,
 *       4 bp_wave with a team per syndrome, 5 the slot kernel.  Launches nothing.  LDPC_HIP_ERR_INVALID: NULL argument or negative batch;
 *       LDPC_HIP_ERR_UNSUPPORTED, with the reason, where a row-prior decode would be refused (a serial schedule, float32 messages, memory,
 *       Relay-BP, guided decimation). */
int ldpc_hip_bp_set_small_code_kernel(ldpc_hip_bp *h, int32_t mode);
int ldpc_hip_bp_row_prior_route(const ldpc_hip_bp *h, int64_t batch, int32_t want_llr, int32_t *route);
/* Measurement / test switches: kernel-shape choices that never change a result (profiles/README.md lists them: "PS_TEAM",
 * "OSD_UNBLOCKED", "OSD_PLANES", "EDGE_STATIC_PCT", "EDGE_CHUNK", ...; for schedule = serial_relative: "REL_LDS" 0 = the
 * per-lane kernel with the state in HBM, 16 / 64 = lanes per syndrome of the on-chip kernel; "REL_LEVELS" 0 = sweep bit by bit instead of
 * level by level; "REL_SCRATCH_IN_L" 0 = scratch apart from the posterior array; "REL_PROF" 1 = print the kernel's cycle shares per phase
 * to stderr; for the streamed serial schedule: "SER_WAVES" / "SER_RING" wavefronts per tile and ring depth, "SER_LANE_MAX" rows at or below
 * which what a pass left finishes a workgroup per syndrome (0 = never), "SER_LANE_THREADS"; "VAR_RING" 1 = the streamed kernel's variable-degree LDS ring wherever it applies (rows <= 16, columns <= 8
 * entries), "VAR_RING_UNITS" its KiB of LDS per wavefront (8 .. 40, default 11); "SPREAD_NODES" rows per wavefront of the
 * per-pass kernels from the start; "SER_VAR" 0 = the streamed serial schedule's item form (any degree profile) never, 1 = also
 * on (6,3)-regular matrices, "SER_VAR_UNITS" its KiB of LDS per wavefront (default 8); "REL_EXT" 0 / 1 = serial_relative's on-chip kernel never / always with the messages and
 * per-entry records in global memory (default: where the all-in-LDS form leaves fewer than four wavefronts per compute unit); "OSD_COLLECT_AFTER" 1 = BP + OSD lists the
 * rows BP left unconverged in a launch of its own after the BP kernel instead of inside the on-chip BP kernels; "OSD_NO_FLAT" 1 = OSD-0 on small matrices without the column permutation (osd0_reg_kernel instead of osd0_flat_kernel); "SPREAD_NT" 0 / 1 = the FP64 per-pass kernels with the default / the non-temporal cache policy whatever the batch size (default: non-temporal beyond 384 MiB of messages in flight); "REPACK_MIN_TILES" t > 0 = the FP64 streamed two-pass decode from t tiles on instead of from 512; "DEM_GRID" k > 0 = dem_sample_b8_kernel launched with at most k workgroups, so its wavefronts loop over shots at any batch size; "F32_NT" 0 / 1 = the float32 per-pass kernels with the default / the non-temporal cache policy whatever the batch size (default: non-temporal beyond 384 MiB of messages in flight); "F32_GRID_ROWS" k > 0 = the four per-round float32 kernels launched with at most k workgroup rows, so that each row loops over several tiles of the list at any batch size (default: all tiles while they are few, else ~16 384 workgroups and at least 256 rows); "F32_ONCHIP" 0 = the float32 mode never takes its on-chip lane = edge kernels (default: on the codes the FP64 lane = edge kernels take, unless one of "F32_NT", "F32_GRID_ROWS", "SPREAD_NODES" is set); "EDGE_CLAMP" 1 = the lane = edge min-sum kernel always
 * with its clamp to DBL_MAX (default: left out where it provably never bites)).  A handle reads the environment variables LDPC_HIP_<NAME> ONCE, when it is
 * created; afterwards only this call changes a switch (value < 0: back to "not set").  Unknown names are an error. */
int ldpc_hip_bp_set_debug_switch(ldpc_hip_bp *h, const char *name, int32_t value);

#define LDPC_HIP_MATH_LIBM_EXACT 0
#define LDPC_HIP_MATH_FAST 1
int ldpc_hip_bp_set_math(ldpc_hip_bp *h, int32_t math_mode);

/*
 * Precision of the messages (opt-in; the default is the reference's FP64 arithmetic, bit for bit).
 *   LDPC_HIP_MSG_F64 (default): every kernel family stores and computes messages in FP64.
 *   LDPC_HIP_MSG_F32: minimum-sum on the parallel schedule with FP32 messages -- half the message traffic.  The priors are the handle's
 *       FP64 log((1 - p) / p) rounded once to FP32; every minimum, multiply by alpha (formed in FP64, rounded once) and addition of the
 *       FP64 kernels is performed as ONE FP32 operation in the same order, no FMA contraction; the posterior is the FP32 sum, the hard
 *       decision `posterior <= 0`; convergence, early exit and iteration counts as in FP64.  The results are NOT the reference's bits:
 *       they are those of this FP32 restatement (tests/f32_util.py), bit for bit.  log-ratios keep their type: each is an FP32
 *       posterior widened exactly.  ldpc_hip_bp_decode_batch[_async], ldpc_hip_bposd0_decode_batch[_async] and
 *       ldpc_hip_bposd_decode_batch[_async] route BP through the FP32 kernels (OSD runs unchanged on the widened posteriors).
 *       Refused with LDPC_HIP_ERR_UNSUPPORTED (ldpc_hip_last_error says why) before anything is staged: product-sum, any serial
 *       schedule, the *_priors entry points, soft-syndrome decoding, and ldpc_hip_bp_multi_decode_batch.
 *       Small codes stay on chip, one launch per decode: the codes of the two lane = edge families (rows <= 4 / columns <= 2, rows <= 8 /
 *       columns <= 4) with the messages in registers; with ldpc_hip_bp_set_f32_lane_node on also the codes beyond them (rows <= 16,
 *       columns <= 8, a syndrome's state within LDS) with the messages in LDS.  Every other code, and every code under small-code kernel
 *       mode 0 or 2, takes the per-pass kernels: four launches an iteration, the messages in HBM.  All routes give the same bits.
 * The setter returns LDPC_HIP_ERR_INVALID for any other value; the getter returns the current value, or LDPC_HIP_ERR_INVALID for NULL.
 *   ldpc_hip_bp_set_f32_lane_node(h, on): on = 1 adds the lane = node kernel (bp_wave_f32_kernel.h: a syndrome's FP32 messages in LDS, one
 *       wavefront or a team -- the workgroup -- per syndrome) to the LDPC_HIP_MSG_F32 routes, for the codes beyond both lane = edge ladders.
 *       Off (0) by default.  A setting of the handle, independent of the message dtype and read only by float32 decodes.  With it on the
 *       route follows ldpc_hip_bp_relay_route's order: small-code kernel modes -1, 1 and 6 ask the lane = edge families first, mode 6 stops
 *       there, modes -1, 1 and 3 take the lane = node kernel's own choice between one wavefront and a team, 4 and 5 force either; modes 0
 *       and 2 stay per-pass.  LDPC_HIP_ERR_INVALID: NULL handle, or a value other than 0 and 1.
 *   ldpc_hip_bp_get_f32_lane_node(h, &on): LDPC_HIP_ERR_INVALID for a NULL argument.
 *   ldpc_hip_bp_f32_route(h, batch, want_llr, &route): which kernels a float32 decode of `batch` syndromes takes on this handle as it is set
 *       now (whatever its current message dtype), with or without log-ratios -- 0 the per-pass kernels, 1 bp_edge, 2 bp_edge8, 3 bp_wave_f32
 *       with one wavefront per syndrome, 4 with a team per syndrome.  Launches nothing.  LDPC_HIP_ERR_INVALID: NULL argument or negative batch.
 */
#define LDPC_HIP_MSG_F64 0
#define LDPC_HIP_MSG_F32 1
int ldpc_hip_bp_set_message_dtype(ldpc_hip_bp *h, int32_t dtype);
int ldpc_hip_bp_get_message_dtype(const ldpc_hip_bp *h);
int ldpc_hip_bp_set_f32_lane_node(ldpc_hip_bp *h, int32_t on);
int ldpc_hip_bp_get_f32_lane_node(const ldpc_hip_bp *h, int32_t *on);
int ldpc_hip_bp_f32_route(const ldpc_hip_bp *h, int64_t batch, int32_t want_llr, int32_t *route);

/*
 * Memory min-sum BP (opt-in; no counterpart in the reference): per-bit memory strengths gamma[n] -- Mem-BP, or with strengths that differ
 * from bit to bit DMem-BP, the building block of Relay-BP.  Minimum-sum, parallel schedule, FP64 messages.  With L0[j] = log((1 - p[j]) / p[j])
 * as the handle forms it and M[b][j] the posterior log-ratio of bit j of syndrome b -- L0[j] to begin with -- the bit pass of iteration it
 * reads, wherever the plain decode reads L0[j] (the forward partial sums and so the posterior),
 *       prior_it[b][j] = L0[j]                              if gamma[j] == 0.0   (a select, no arithmetic)
 *                      = a[j] + gamma[j] * M_prev[b][j]     otherwise,           a[j] = (1.0 - gamma[j]) * L0[j] formed once on the host
 * with every product and sum rounded on its own (no FMA); M_prev is the posterior the previous iteration's bit pass computed for that row.
 * The check pass, the scaling factor (0 included), the initial messages L0[j], the convergence test and the freezing of a converged row's
 * outputs are the plain decode's.  gamma all zero gives the plain decode's bits.  The results are those of the NumPy restatement
 * tests/mem_bp_util.py, bit for bit.
 *   ldpc_hip_bp_set_memory(h, gamma): gamma = host pointer to [n], each finite and in [-1, 1) (else LDPC_HIP_ERR_INVALID); NULL = off (the
 *       plain decode and its kernels again).  ldpc_hip_bp_set_channel afterwards is followed: a[] is formed again.
 *   ldpc_hip_bp_get_memory(h, out): 1 if memory is on (gamma copied to out[n] unless out is NULL), 0 if off, LDPC_HIP_ERR_INVALID for NULL.
 * With memory on, ldpc_hip_bp_decode_batch[_async], the BP + OSD entry points, ldpc_hip_bp_decode_b8 and ldpc_hip_bp_simulate_b8 decode
 * with it (OSD runs unchanged on the posteriors).  Refused with LDPC_HIP_ERR_UNSUPPORTED (ldpc_hip_last_error says why) before anything is
 * staged or launched: product-sum, any serial schedule, LDPC_HIP_MSG_F32, the *_priors entry points, soft-syndrome decoding -- and, at
 * decode time against the priors the handle holds then, a nonzero gamma[j] on a column whose channel probability is 0 or 1 (it needs
 * probabilities strictly between 0 and 1; columns with gamma[j] == 0 may keep theirs).
 */
int ldpc_hip_bp_set_memory(ldpc_hip_bp *h, const double *gamma);
int ldpc_hip_bp_get_memory(const ldpc_hip_bp *h, double *out);

/*
 * Relay-BP (opt-in; no counterpart in the reference): `legs` memory min-sum legs chained per syndrome and decoded in one call.  Leg l runs at
 * most leg_iters[l] iterations with the strengths gamma[l][0 .. n) -- leg_iters takes the place of the handle's max_iter -- exactly as the memory
 * decode above iterates (a scaling factor of 0 counts the LEG's iterations), with two differences from the second leg on: M starts as the
 * posteriors the previous leg ended with (of its last bit pass: the iteration it converged at, or its last), and the initial bit-to-check
 * message of every entry of column j is gamma[l][j] == 0 ? L0[j] : a[l][j] + gamma[l][j] * M[j] (the product rounded, then the sum).
 * A leg that reproduces the syndrome is a solution; its weight is the sum of L0[j] over its decided bits, an FP64 sum in one fixed order
 * (relay_common.h: relay_weight).  The row stops after stop_after solutions.  Outputs: the lightest solution -- the first among equal weights --
 * with the posteriors of its leg, converge = 1; a row without any solution gets the last leg's last decisions and posteriors, converge = 0;
 * iterations = the sum over the legs the row ran.  A syndrome byte > 1 never converges.  The results are those of the NumPy restatement
 * tests/relay_bp_util.py, bit for bit, on every route (ldpc_hip_bp_relay_route names the one a handle takes): the lane = edge relay kernels (all
 * legs in one launch, nothing leaves the chip between legs) for the codes those kernels take, the lane = node kernel bp_wave_relay_kernel (the
 * same, messages and memory in LDS) where the small-code kernel mode asks for it, and otherwise a loop of per-pass memory decodes with a selection
 * kernel after each leg (correct everywhere, not fast); nothing is read back between legs, so the *_async entry points stay asynchronous.
 *   ldpc_hip_bp_set_relay(h, legs, gamma, leg_iters, stop_after): gamma = host pointer to [legs * n], each finite and in [-1, 1); leg_iters =
 *       host pointer to [legs], each >= 1; stop_after >= 1 (else LDPC_HIP_ERR_INVALID).  legs = 0 or gamma = NULL: off.  Relay and
 *       ldpc_hip_bp_set_memory exclude each other: setting one while the other is on is LDPC_HIP_ERR_UNSUPPORTED.  ldpc_hip_bp_set_channel
 *       afterwards is followed: a[] of every leg is formed again.
 *   ldpc_hip_bp_get_relay(h, &legs, &stop_after, gamma_out, leg_iters_out): 1 if the relay is on (legs and stop_after set; gamma_out[legs * n]
 *       and leg_iters_out[legs] filled unless NULL), 0 if off (legs = stop_after = 0), LDPC_HIP_ERR_INVALID for a NULL handle.
 * With the relay on, ldpc_hip_bp_decode_batch[_async], the BP + OSD-0 entry points (OSD sees the rows the relay leaves without a solution, with
 * the last leg's posteriors), ldpc_hip_bp_decode_b8 and ldpc_hip_bp_simulate_b8 decode with it.  Refused with LDPC_HIP_ERR_UNSUPPORTED before
 * anything is staged or launched: product-sum, any serial schedule, LDPC_HIP_MSG_F32, the *_priors entry points, soft-syndrome decoding,
 * several GPUs, OSD-E / OSD-CS -- and, at decode time, a nonzero gamma[l][j] in any leg on a column whose channel probability is 0 or 1.
 */
int ldpc_hip_bp_set_relay(ldpc_hip_bp *h, int32_t legs, const double *gamma, const int32_t *leg_iters, int32_t stop_after);
int ldpc_hip_bp_get_relay(const ldpc_hip_bp *h, int32_t *legs, int32_t *stop_after, double *gamma_out, int32_t *leg_iters_out);

/* Which kernel route a Relay-BP or memory min-sum decode of `batch` syndromes takes on this handle as it is set now (code, small-code kernel mode):
 *   0  the per-pass kernels (Relay-BP: the leg loop -- legs x iterations x four launches over every tile; correct everywhere, not fast)
 *   1  bp_edge: lane = edge, rows <= 4, columns <= 2         2  bp_edge8: lane = edge, rows <= 8, columns <= 4
 *   3  bp_wave: lane = node, messages and memory in LDS, one wavefront per syndrome      4  bp_wave, a whole workgroup (team) per syndrome
 * Routes 1 - 4 run all legs of a syndrome in one launch; the results are the same bits on every route.  Launches nothing.
 * LDPC_HIP_ERR_INVALID: NULL argument, negative batch, or neither ldpc_hip_bp_set_relay nor ldpc_hip_bp_set_memory is on. */
int ldpc_hip_bp_relay_route(const ldpc_hip_bp *h, int64_t batch, int32_t *route);

/*
 * BP with guided decimation, BPGD (opt-in; no counterpart in the reference): minimum-sum, parallel schedule, FP64 messages, in up to max_rounds
 * rounds of up to round_iters iterations per syndrome -- the two take the place of the handle's max_iter.  With L0[j] = log((1 - p[j]) / p[j]),
 * P = L0 and frozen[j] = !isfinite(L0[j]) to start with, every iteration is the plain decode's with P for the prior; the iteration count runs on
 * across the rounds (a scaling factor of 0 takes alpha = 1 - 2^-it of the row's TOTAL it), and the first iteration whose decisions reproduce the
 * syndrome ends the row: converge = 1, iterations = it.  A round that ends without that, and is not the last, decimates: with M the posteriors of
 * its last bit pass, j* = the column with frozen[j] false and M[j] not NaN whose |M[j]| is largest (the smallest j among equal ones) gets
 * v = M[j*] <= 0 ? -freeze_llr : +freeze_llr for its prior P[j*] and for every one of its bit-to-check messages, and is frozen; every other
 * message stays.  With nothing left to freeze the rounds still run.  A row that never converges: the last bit pass, converge = 0, iterations =
 * max_rounds * round_iters.  A syndrome byte > 1 never converges.  max_rounds = 1 is the plain decode with max_iter = round_iters, bit for bit.
 * The results are those of the NumPy restatement tests/bpgd_util.py, bit for bit.
 *   ldpc_hip_bp_set_decimation(h, round_iters, max_rounds, freeze_llr): round_iters >= 1, max_rounds >= 1, their product within int32,
 *       freeze_llr > 0 and finite or +inf (else LDPC_HIP_ERR_INVALID, the message names the value, and what the handle held stays).
 *       round_iters = 0: off.  Decimation, ldpc_hip_bp_set_relay and ldpc_hip_bp_set_memory exclude one another: setting one while another is on
 *       is LDPC_HIP_ERR_UNSUPPORTED.  ldpc_hip_bp_set_channel afterwards is followed.
 *   ldpc_hip_bp_get_decimation(h, &round_iters, &max_rounds, &freeze_llr): 1 if it is on (the three set unless NULL), 0 if off (all three 0),
 *       LDPC_HIP_ERR_INVALID for a NULL handle.
 *   ldpc_hip_bp_decimation_route(h, batch, &route): which kernels decode `batch` syndromes with it on this handle as it is set now -- 0 none,
 *       1 bp_edge (lane = edge, rows <= 4, columns <= 2), 2 bp_edge8 (rows <= 8, columns <= 4), and with the lane = node switch on 3 bp_wave_gd
 *       with one wavefront per syndrome, 4 with a team (the workgroup) per syndrome.  Launches nothing.  LDPC_HIP_ERR_INVALID: NULL argument,
 *       negative batch, or the decimation is off.
 *   ldpc_hip_bp_set_decimation_lane_node(h, on): on = 1 adds the lane = node kernel (bp_wave_gd_kernel.h: a syndrome's messages, posteriors and
 *       frozen columns in LDS, one wavefront or a team per syndrome, all rounds in one launch) for the codes beyond both lane = edge ladders:
 *       rows <= 16, columns <= 8, a syndrome's state within LDS.  Off (0) by default.  A setting of the handle, independent of whether the
 *       decimation is on and read only while it is.  With it on the route follows ldpc_hip_bp_relay_route's order: any small-code kernel mode
 *       but 0 asks the lane = edge families first, mode 6 stops there, modes -1, 1 and 3 take the lane = node kernel's own choice between one
 *       wavefront and a team, 4 and 5 force either.  LDPC_HIP_ERR_INVALID: NULL handle, or a value other than 0 and 1.
 *   ldpc_hip_bp_get_decimation_lane_node(h, &on): LDPC_HIP_ERR_INVALID for a NULL argument.
 * The lane = edge kernels (bp_edge_gd_kernel.h: one wavefront per syndrome, all rounds in one launch, nothing leaves the chip between rounds) are
 * the only route unless the lane = node switch is on; a per-pass route is not built.  With the decimation on,
 * ldpc_hip_bp_decode_batch[_async], the BP + OSD-0 entry points (OSD sees the rows left unsolved, with the last posteriors), ldpc_hip_bp_decode_b8
 * and ldpc_hip_bp_simulate_b8 decode with it.  Refused with LDPC_HIP_ERR_UNSUPPORTED before anything is staged or launched: a code no route
 * takes under the small-code kernel mode (route 0: with the switch off, a code neither lane = edge family takes or a mode other than -1, 1, 6),
 * product-sum, any serial schedule, LDPC_HIP_MSG_F32, the *_priors entry points, soft-syndrome decoding, several GPUs, OSD-E / OSD-CS.
 */
int ldpc_hip_bp_set_decimation(ldpc_hip_bp *h, int32_t round_iters, int32_t max_rounds, double freeze_llr);
int ldpc_hip_bp_get_decimation(const ldpc_hip_bp *h, int32_t *round_iters, int32_t *max_rounds, double *freeze_llr);
int ldpc_hip_bp_decimation_route(const ldpc_hip_bp *h, int64_t batch, int32_t *route);
int ldpc_hip_bp_set_decimation_lane_node(ldpc_hip_bp *h, int32_t on);
int ldpc_hip_bp_get_decimation_lane_node(const ldpc_hip_bp *h, int32_t *on);

/* The shader clock the BP kernels actually ran at (a measurement aid; no counterpart in the reference).  Every workgroup of the
 * long-running BP kernels (bp_decode_kernel, bp_wave_kernel, bp_wave_ps_kernel, bp_edge_kernel, bp_edge8_kernel) adds the shader cycles
 * (s_memtime) and the constant-rate ticks (s_memrealtime) of its lifetime to two 64-bit words of the handle; the words only grow.
 * This call waits for the handle's stream and returns them together with the tick rate (hipDeviceAttributeWallClockRate).
 * Clock over an interval = (cycles_after - cycles_before) / (ticks_after - ticks_before) * tick_hz, averaged over the kernels'
 * workgroups and weighted by their lifetime. */
int ldpc_hip_bp_clock_probe(ldpc_hip_bp *h, uint64_t *cycles, uint64_t *ticks, double *tick_hz);

/* The copy rate of THIS box, now (a measurement aid; no counterpart in the reference).  Copies `tiles` x `segments_per_tile` segments of
 * 512 bytes (64 syndromes x one double: the unit every streamed BP kernel moves) from one of the handle's message arrays to the other and
 * back, `passes` times, one workgroup per tile, non-temporal, on the handle's stream, timed with events on that stream.
 * gbytes_per_s = bytes read + bytes written per second.  bench.py prints it beside the roofline fraction so that one JSON line tells a slow
 * box from a slow build: boxes of the pool differ by ~10 % in what they give ANY kernel that moves these bytes once.  The handle's
 * message arrays are (re)allocated to the probe's size if they are smaller; their contents are scratch between decodes anyway. */
int ldpc_hip_bp_copy_probe(ldpc_hip_bp *h, int64_t tiles, int32_t segments_per_tile, int32_t passes, float *ms, double *gbytes_per_s);

/* Bytes of device memory the library's grow-only buffers hold right now, over every handle of the process (a test aid; no counterpart in
 * the reference): workspaces, staging and the tables built on first use -- not the matrix and priors a handle uploads when it is created.
 * A handle's share is gone once ldpc_hip_bp_destroy returns. */
int64_t ldpc_hip_debug_device_buf_bytes(void);

/* Launch log (a test aid; no counterpart in the reference): which kernel instantiations the library launched, over every handle and thread
 * of the process.  ldpc_hip_debug_launch_log(1) empties the table and starts recording, (0) stops AND empties it -- read before disabling; off -- the default -- a launch costs one
 * load of a flag.  ldpc_hip_debug_launch_log_read copies the table as text, one "count<TAB>name" line per instantiation in the spelling
 * of tools/list_instantiations.py ("bp_edge8_kernel<12, 3, true>"), NUL-terminated and cut to `capacity` bytes, and returns the bytes the
 * whole text needs (call it with capacity 0 first).  The environment variable LDPC_HIP_LAUNCH_LOG=<file>, read when the library is loaded,
 * records for the whole process and appends its table to the file at unload (profiles/README.md); the calls here do not disturb it. */
void ldpc_hip_debug_launch_log(int32_t enable);
int64_t ldpc_hip_debug_launch_log_read(char *buf, int64_t capacity);

/* Math probe (a test aid; no counterpart in the reference): out[i] = f(in[i]) with f one of the inline routines of csrc/bp_math.h, evaluated
 * ON THE DEVICE by one small kernel that calls the routines the decode kernels call -- so the device compile of them (the hand-rolled division,
 * the inline-assembly fma, the wavefront ballot in front of every rare tail) can be compared with the host compile argument by argument.
 *   which  0 tanh_half_libm   1 log_libm   2 ps_log_ratio_libm   3 log_near_one(q) ? log_libm_near_one(q) : log_libm_general(q, table)
 *          4 div_cr: out[i] = div_cr(in[2 i], in[2 i + 1]) (`in` holds 2 count doubles)   5 tanh_half   6 ps_log_ratio
 * Fixed layout: elements 64 w .. 64 w + 63 are the 64 lanes of ONE wavefront (256-thread blocks, a grid step that is a multiple of 64), so a
 * caller chooses which arguments share a ballot.  Device pointers only, as for ldpc_hip_pack_b8; needs no handle: the kernel is queued on the
 * null stream of the current device without synchronisation. */
int ldpc_hip_debug_math_eval(int32_t which, const double *in, int64_t count, double *out);

/* Page-locked host memory for a caller's result arrays (no counterpart in the reference: its arrays never leave the host).  A host
 * pointer into such a block -- or into memory the caller registered with hipHostRegister -- handed to ldpc_hip_bp_decode_batch as `llr`
 * is written by the device-to-host copies themselves: the pipelined host path (above) skips its pinned staging buffer and the
 * host-side copy for that array.  At 65 536 x 10 000 that is 5.2 GB less to move per call.  NULL when the memory cannot be had
 * (page-locked memory is a limited resource): fall back to ordinary memory. */
void *ldpc_hip_host_alloc(size_t bytes);
void ldpc_hip_host_free(void *p);

const char *ldpc_hip_last_error(void);
const char *ldpc_hip_version(void);

/*
 * ---- several GPUs, one process --------------------------------------------------------------------------------
 * "device_ids[ndev] ... the library owns device memory, streams and the inter-GPU traffic
 * inside the handle".  ldpc_hip_bp_multi_create builds one ordinary handle per entry of device_ids (a device may be
 * listed more than once: two handles then share that GPU); ldpc_hip_bp_multi_decode_batch cuts the batch into
 * contiguous row ranges on 64-syndrome boundaries, decodes every range on its GPU concurrently (one host thread per
 * GPU for the duration of the call) and returns when all results are in the caller's buffers -- row b of every output
 * is what the single-GPU call gives for row b, bit for bit.  Buffers: all host memory (every GPU copies its own rows
 * over its own PCIe link), or all on ONE GPU (the others receive their rows by peer copy over xGMI and send their hard
 * decisions back bit-packed, 1/8 of the bytes, to be unpacked on that GPU when it is one of device_ids).
 * with_osd: -1 = ldpc_hip_bp_decode_batch, 0 = ldpc_hip_bposd0_decode_batch, 1 = ldpc_hip_bposd_decode_batch.
 * Settings (channel, parameters, schedule, OSD, math ...) are applied per GPU through ldpc_hip_bp_multi_handle(mh, i),
 * i < ldpc_hip_bp_multi_devices(mh): the setters above, unchanged.  The schedules that keep state in the decoder object
 * (serial_relative, the random serial schedule) have ONE state per multi handle: a call starts every row from the state of
 * handle 0 (copied to the others first -- which also settles random_schedule_seed = 0, the clock) and leaves the state of the
 * batch's last row on EVERY handle, so that sequences of calls equal the single-GPU sequences bit for bit.  Soft-syndrome
 * decoding (ldpc_hip_bp_soft_info_decode_batch) is a per-handle call: use ldpc_hip_bp_multi_handle(mh, 0).  Multi-PROCESS sharding (one rank per GPU, RCCL
 * gather of the packed rows) is ldpc_amd/sharding.py + bench.py; the reference has neither (bp.hpp:129-140).
 */
typedef struct ldpc_hip_bp_multi ldpc_hip_bp_multi;
int ldpc_hip_bp_multi_create(const ldpc_hip_bp_desc *desc /* desc->device is ignored */, const int32_t *device_ids,
                             int32_t ndev, ldpc_hip_bp_multi **out);
void ldpc_hip_bp_multi_destroy(ldpc_hip_bp_multi *mh);
int32_t ldpc_hip_bp_multi_devices(const ldpc_hip_bp_multi *mh);
ldpc_hip_bp *ldpc_hip_bp_multi_handle(ldpc_hip_bp_multi *mh, int32_t i);
int ldpc_hip_bp_multi_decode_batch(ldpc_hip_bp_multi *mh, int32_t with_osd, const uint8_t *syndromes, int64_t batch,
                                   uint8_t *decoding, double *llr, int32_t *iterations, uint8_t *converge);
/* BP kernel time of the last decode on every GPU (ldpc_hip_bp_last_kernel_ms per handle), ms_per_device[ndev] */
int ldpc_hip_bp_multi_last_kernel_ms(ldpc_hip_bp_multi *mh, float *ms_per_device);
/* Testing aid: force != 0 routes device buffers through the peer-copy / bit-packed path even on the GPU they live on
 * (so that the path can be exercised on a one-GPU machine, e.g. with device_ids = {0, 0}). */
int ldpc_hip_bp_multi_set_staging(ldpc_hip_bp_multi *mh, int32_t force);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_HIP_H */
