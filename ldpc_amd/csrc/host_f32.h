// host_f32.h -- host side of the float32 message mode (bp_f32_kernels.h): its workspace, a chunk's rounds queued
// Part of libldpc_hip.so: included by tu_f32.hip.  Modelled on the per-pass route of host_stream.h (StreamPlan::rp): per-pass kernels
// from the first iteration for any batch size, every round queued without waiting for the device.
#pragma once

// bytes of a 64-syndrome tile: both message arrays, the posteriors if wanted, packed syndromes and decisions
static size_t f32_tile_bytes(const ldpc_hip_bp *h, bool want_llr) {
    const size_t msg = sizeof(float) * (size_t)(h->nnz ? h->nnz : 1) * LDPC_WAVE, post = sizeof(float) * (size_t)(h->n ? h->n : 1) * LDPC_WAVE;
    return 2 * msg + (want_llr ? post : 0) + 16 * (size_t)(h->m + h->n + 1);
}

struct F32Kernels { void (*check)(const F32Args); void (*bit)(const F32Args); };
static F32Kernels pick_f32(const ldpc_hip_bp *h, bool nt) {
    F32Kernels k;
    if (nt) {
        k.check = h->max_row_deg <= 8 ? bp_f32_check_kernel<8, 1> : bp_f32_check_kernel<16, 1>;
        k.bit = h->max_col_deg <= 4 ? bp_f32_bit_kernel<4, 1> : bp_f32_bit_kernel<8, 1>;
    } else {
        k.check = h->max_row_deg <= 8 ? bp_f32_check_kernel<8, 0> : bp_f32_check_kernel<16, 0>;
        k.bit = h->max_col_deg <= 4 ? bp_f32_bit_kernel<4, 0> : bp_f32_bit_kernel<8, 0>;
    }
    return k;
}

// What a float32 pass is told (the analogue of StreamPass, host_stream.h).  Default: a plain decode to h->max_iter.  decode_f32_repacked builds a
// first pass that stops at `end` and leaves its messages behind, and the continuation that carries on the rows it left: known to the device only
// -- `batch` is the most there can be, the kernels read the real count (rows_dev) and reach the caller's rows through row_map; the grids of
// its kernels follow an estimate (they all loop).
struct F32Pass {
    int end = -1;                         // iteration at which the pass's tiles end (-1: the handle's max_iter).  end < max_iter IS "keep the state": a first
                                          // pass, whose last bit pass leaves the messages behind (F32Args::pass_end; no flag of its own as in StreamPass)
    int round0 = 0;                       // continuation: rounds its rows have behind them
    const int32_t *row_map = nullptr;     // ... its rows in the caller's arrays (F32Args::row_map)
    const unsigned *rows_dev = nullptr;   // ... {rows, tiles} on the device (F32Args::rows_dev)
    int64_t grid_tiles = 0;               // ... tiles its grids are sized for (an estimate)
    bool swapped = false;                 // ... bit_to_check lives in h->msgC (gathered there from h->msgA), check_to_bit in h->msgA
    bool continues() const { return rows_dev != nullptr; }
};

// tiles per chunk of a float32 decode of tiles_total tiles
static int f32_chunk_tiles(const ldpc_hip_bp *h, int64_t tiles_total, bool want_llr, int64_t *chunk) {
    return chunk_tiles_that_fit(h, tiles_total, f32_tile_bytes(h, want_llr), h->msgA.cap + h->msgC.cap + h->llr_t.cap, 0.85, 32768, "syndrome", chunk);
}

// One pass over the batch, chunk by chunk: device pointers, on h->stream; `llr` receives FP64 values, each an FP32 posterior widened.
// *chunk_tiles (if asked for): the tiles per chunk it used (== all of them: the whole batch's message state is resident).
static int decode_f32_pass(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv,
                           const F32Pass &pass, int64_t *chunk_tiles = nullptr) {
    int rc;
    const int64_t tiles_total = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    const size_t m1 = (size_t)(h->m ? h->m : 1), n1 = (size_t)(h->n ? h->n : 1), nnz1 = (size_t)(h->nnz ? h->nnz : 1);
    const size_t per_tile_msg = sizeof(float) * nnz1 * LDPC_WAVE, per_tile_llr = llr ? sizeof(float) * n1 * LDPC_WAVE : 0;
    const int pass_end = pass.end < 0 ? h->max_iter : pass.end;
    int64_t chunk = 0;
    if ((rc = f32_chunk_tiles(h, tiles_total, llr != nullptr, &chunk))) return rc;
    if (pass.continues() && chunk < tiles_total) return fail(LDPC_HIP_ERR_NOMEM, "internal: the second pass of a compacted float32 decode must be one chunk");
    if (chunk_tiles) *chunk_tiles = chunk;
    const size_t ct = (size_t)chunk;
    // (nzm: no float32 kernel reads it -- min-sum needs the parity word and the invalid mask only; it exists because pack_syndromes_kernel writes it)
    if ((rc = h->msgA.ensure(per_tile_msg * ct)) || (rc = h->msgC.ensure(per_tile_msg * ct))) return rc;
    if ((rc = h->par.ensure(sizeof(uint64_t) * m1 * ct)) || (rc = h->nzm.ensure(sizeof(uint64_t) * m1 * ct)) || (rc = h->invalid.ensure(sizeof(uint64_t) * ct))) return rc;
    if ((rc = h->dec.ensure(sizeof(uint64_t) * n1 * ct)) || (rc = h->dcur.ensure(sizeof(uint64_t) * n1 * ct))) return rc;
    if (per_tile_llr && (rc = h->llr_t.ensure(per_tile_llr * ct))) return rc;
    if ((rc = h->tile_state.ensure(sizeof(TileState) * ct)) || (rc = h->handoff_list.ensure(sizeof(int32_t) * ct)) || (rc = h->counter.ensure(16))) return rc;
    if ((rc = h->f32_llr0.ensure(sizeof(float) * n1))) return rc;
    reset_timing(h, false);  // (a second pass keeps the first pass's events, timed_prev: ldpc_hip_bp_last_kernel_ms adds them)
    hipStream_t st = h->stream;
    if (h->n > 0 && !pass.continues())  // (a second pass: the first pass's are there)
        LDPC_LAUNCH(bp_f32_priors_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, st, (const double *)h->d_llr0, h->n, (float *)h->f32_llr0.p);
    HIPCHK(hipGetLastError());
    for (int64_t t0 = 0; t0 < tiles_total; t0 += chunk) {
        const ChunkRange c = chunk_range(t0, chunk, tiles_total, batch);
        const unsigned tiles = (unsigned)c.tiles;
        // tiles the grids are sized for: a continuation's estimate (its kernels loop over what the device counts), else the chunk's
        const unsigned loop_tiles = pass.continues() ? (unsigned)(pass.grid_tiles < c.tiles ? (pass.grid_tiles > 0 ? pass.grid_tiles : 1) : c.tiles) : tiles;
        HIPCHK(hipMemsetAsync(h->invalid.p, 0, sizeof(uint64_t) * (size_t)c.tiles, st));
        HIPCHK(hipMemsetAsync(h->dec.p, 0, sizeof(uint64_t) * n1 * (size_t)c.tiles, st));
        HIPCHK(hipMemsetAsync(h->counter.p, 0, 16, st));
        if (h->m > 0)
            LDPC_LAUNCH(pack_syndromes_kernel, dim3((unsigned)((h->m + 255) / 256), loop_tiles), dim3(256), 0, st, synd + c.b0 * h->m, c.nb, h->m,
                               (uint64_t *)h->par.p, (uint64_t *)h->nzm.p, (uint64_t *)h->invalid.p, pass.row_map, pass.rows_dev);
        HIPCHK(hipGetLastError());
        F32Args a = {};
        a.m = h->m; a.n = h->n; a.nnz = h->nnz; a.max_iter = h->max_iter; a.pass_end = pass_end; a.round0 = pass.round0;
        a.ms_scaling_factor = h->ms_scaling_factor; a.batch = c.nb;
        a.row_map = pass.row_map; a.rows_dev = pass.rows_dev;
        a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx; a.col_ptr = h->d_col_ptr; a.csc_edge = h->d_csc_edge;
        a.llr0 = (const float *)h->f32_llr0.p;
        a.A = (float *)(pass.swapped ? h->msgC.p : h->msgA.p); a.C = (float *)(pass.swapped ? h->msgA.p : h->msgC.p);
        a.par = (const uint64_t *)h->par.p; a.invalid = (const uint64_t *)h->invalid.p;
        a.dec = (uint64_t *)h->dec.p; a.dcur = (uint64_t *)h->dcur.p;
        a.llr_t = per_tile_llr ? (float *)h->llr_t.p : nullptr;
        a.iters = iters ? iters + c.b0 : nullptr; a.conv = conv ? conv + c.b0 : nullptr;
        a.state = (TileState *)h->tile_state.p; a.counters = (unsigned *)h->counter.p; a.list = (int32_t *)h->handoff_list.p;
        a.host_flag = h->d_flag;
        a.seq = ++h->flag_seq ? h->flag_seq : ++h->flag_seq;  // never 0 (the word's initial value); a fresh one per pass
        // rows (columns) per wavefront, as the FP64 per-pass route chooses them (host_stream.h: stream_start_per_pass)
        a.nodes = h->sw("SPREAD_NODES") > 0 ? h->sw("SPREAD_NODES") : loop_tiles <= 8 ? 1 : loop_tiles < 512 ? 4 : 16;
        if ((rc = chunk_timing_begin(h))) return rc;
        LDPC_LAUNCH(bp_f32_state_init_kernel, dim3((tiles + 255) / 256), dim3(256), 0, st, a, (int)tiles);
        if (pass.continues()) {
            // the listed rows' bit_to_check state after the first pass (h->msgA), lane by lane, into dense tiles (h->msgC: this pass's A)
            const int epw = 16;
            const dim3 gg((unsigned)((h->nnz + 4 * epw - 1) / (4 * epw)), loop_tiles);
            LDPC_LAUNCH(bp_f32_gather_lanes_kernel, gg, dim3(256), 0, st, (const float *)a.C, pass.row_map, pass.rows_dev, h->nnz, epw, a.A);
        } else {
            LDPC_LAUNCH(bp_f32_init_kernel, dim3((unsigned)(h->nnz ? (h->nnz + 63) / 64 : 1), tiles), dim3(256), 0, st, a);
        }
        HIPCHK(hipGetLastError());
        // Every kernel of a round loops over the listed tiles, so a launch needs only enough workgroup rows to fill the chip: all the
        // tiles while they are few, else what gives ~16 384 workgroups (at least 256 rows).  Once tiles have finished the list is
        // compacted every 4 rounds and the rows beyond it leave at once.
        // (switch F32_GRID_ROWS k > 0: at most k rows for all four kernels -- the tests reach gridDim.y < count at 70 tiles with it)
        const int grid_rows = h->sw("F32_GRID_ROWS");
        auto rows_for = [&](unsigned gx) {
            const unsigned want = grid_rows > 0 ? (unsigned)grid_rows : 16384u / gx > 256u ? 16384u / gx : 256u;
            return loop_tiles < want ? loop_tiles : want;
        };
        const unsigned per_wg = 4u * (unsigned)a.nodes;
        const unsigned gcx = (unsigned)(h->m ? (h->m + per_wg - 1) / per_wg : 1), gbx = (unsigned)(h->n ? (h->n + per_wg - 1) / per_wg : 1);
        const unsigned gsx = (unsigned)(h->m ? (h->m + 255) / 256 : 1), gfx = (unsigned)(h->n ? (h->n + 63) / 64 : 1);
        // messages of the tiles in flight beyond ~the MALL are streamed, not cached (as stream_rounds decides it)
        // (switch F32_NT 0 / 1: the policy whatever the size -- the tests run the non-temporal instantiations on a small case with it)
        const bool nt = h->sw("F32_NT") >= 0 ? h->sw("F32_NT") > 0 : (double)loop_tiles * 2.0 * (double)per_tile_msg > 384.0 * 1024.0 * 1024.0;
        const F32Kernels k = pick_f32(h, nt);
        const volatile unsigned *flag = h->h_flag;
        // The tile list is compacted every 4 rounds OF THE PASS from its 4th on -- a plain decode and a first pass at rounds 4, 8, ... as
        // ever, a second pass at round0 + 4, round0 + 8, ...: its tiles are dense with rows that were all still decoding at round0, so its
        // list thins out by the same clock a fresh decode's does, counted from its own start.
        for (int round = pass.round0; round < pass_end; ++round) {
            if (*flag == a.seq) break;  // a look, not a wait: the device has reported the last tile final
            a.round = round;
            const int r = round - pass.round0;
            if (r >= 4 && r % 4 == 0) LDPC_LAUNCH(bp_f32_compact_kernel, dim3(1), dim3(64), 0, st, a);
            LDPC_LAUNCH(k.check, dim3(gcx, rows_for(gcx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(k.bit, dim3(gbx, rows_for(gbx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(bp_f32_synd_kernel, dim3(gsx, rows_for(gsx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(bp_f32_finish_kernel, dim3(gfx, rows_for(gfx)), dim3(256), 0, st, a);
        }
        HIPCHK(hipGetLastError());
        if ((rc = chunk_timing_end(h))) return rc;
        if (h->n > 0) {
            LDPC_LAUNCH(unpack_decoding_kernel, dim3((unsigned)((h->n + 255) / 256), loop_tiles), dim3(256), 0, st, (const uint64_t *)h->dec.p, c.nb, h->n,
                               decoding + c.b0 * h->n, pass.row_map, pass.rows_dev);
            if (llr)
                LDPC_LAUNCH(bp_f32_transpose_llr_kernel, dim3((unsigned)((h->n + LDPC_WAVE - 1) / LDPC_WAVE), loop_tiles), dim3(256), 0, st,
                                   (const float *)h->llr_t.p, c.nb, h->n, llr + (size_t)c.b0 * h->n, pass.row_map, pass.rows_dev);
        }
        HIPCHK(hipGetLastError());
    }
    return LDPC_HIP_OK;
}

// Two passes, as decode_stream_repacked (host_stream.h) does it for FP64: k1 iterations for every row, then the rows still decoding are
// compacted -- their bit_to_check state gathered lane by lane into dense tiles (bp_f32_gather_lanes_kernel) -- and the decode carries on from
// iteration k1 + 1 on those: the same operations on the same values in the same order, so every row gets the bits of the plain decode.
// k1: ldpc_hip_bp_set_repack -- forced, or priced on the histogram the previous decode left (stream_first_pass_length; the float32 round
// also moves four message-array passes, so the gather costs 0.25 of an iteration here too).  Nothing waits for the device: the second pass
// is queued at once, its grids sized from the histogram's estimate, and it learns its rows on the device (osd_collect_kernel lists them,
// repack_rows_kernel turns the count into {rows, tiles}, F32Args::rows_dev / row_map).  No extra message memory: the gather writes into the
// first pass's check_to_bit array, dead by then, and the second pass uses the two arrays with their roles swapped.  The first pass's
// outputs are unpacked and transposed before the second pass reuses dec, dcur, llr_t, par, the tile states and the tile list: stream order.
static int decode_f32_repacked(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    const int full = h->max_iter;
    const size_t B = (size_t)batch;
    int rc;
    if (!conv) { if ((rc = h->osd_conv.ensure(B))) return rc; conv = (uint8_t *)h->osd_conv.p; }
    if (!iters) { if ((rc = h->sp_iters.ensure(B * 4))) return rc; iters = (int32_t *)h->sp_iters.p; }
    double live = 0.5;
    int64_t late_rows = -1;  // (what the FP64 second pass sizes its late rounds by; every float32 kernel loops over a compacted list anyway)
    int k1 = stream_first_pass_length(h, &live, &late_rows, 0.25);
    const int64_t tiles1 = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    if (k1 >= 2 && k1 < full) {
        // the compaction needs the whole batch's message state resident (one chunk); else decode plainly
        int64_t chunk = 0;
        if ((rc = f32_chunk_tiles(h, tiles1, llr != nullptr, &chunk))) return rc;
        if (chunk < tiles1 || h->nnz == 0) k1 = 0;
    }
    if (k1 >= 2 && k1 < full) {
        F32Pass first;
        first.end = k1;
        int64_t chunk1 = 0;
        if ((rc = decode_f32_pass(h, synd, batch, decoding, llr, iters, conv, first, &chunk1))) return rc;
        // (else the first pass was cut into chunks after all -- free memory moved between the estimate above and its own: there is nothing
        // to compact -- decode the batch plainly: same results; the first pass's work is lost)
        if (chunk1 < tiles1) k1 = 0;
    }
    if (k1 < 2 || k1 >= full) {
        if ((rc = decode_f32_pass(h, synd, batch, decoding, llr, iters, conv, F32Pass()))) return rc;
        return stream_leave_histogram(h, iters, conv, batch);
    }
    if ((rc = h->osd_list.ensure(B * sizeof(int32_t))) || (rc = h->osd_counters.ensure(4 * sizeof(unsigned)))) return rc;  // {count, next, rows, tiles}
    HIPCHK(hipMemsetAsync(h->osd_counters.p, 0, 4 * sizeof(unsigned), h->stream));
    LDPC_LAUNCH(osd_collect_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, conv, batch,
                       (int32_t *)h->osd_list.p, (unsigned *)h->osd_counters.p, (uint8_t *)nullptr);
    LDPC_LAUNCH(repack_rows_kernel, dim3(1), dim3(1), 0, h->stream, (const unsigned *)h->osd_counters.p, (unsigned *)h->osd_counters.p + 2);
    HIPCHK(hipGetLastError());
    // the first pass's events stay readable while the second pass records its own (ldpc_hip_bp_last_kernel_ms adds both; nobody waits here)
    std::swap(h->ev0, h->evp0); std::swap(h->ev1, h->evp1);
    h->timed_prev = h->timed; h->timed_prev_mid = false;
    F32Pass second;
    second.round0 = k1; second.swapped = true;
    second.row_map = (const int32_t *)h->osd_list.p; second.rows_dev = (const unsigned *)h->osd_counters.p + 2;
    // grids: the rows the histogram expects + a margin (the kernels loop, so any count is handled)
    second.grid_tiles = (int64_t)(live * 1.25 * (double)tiles1) + 8;
    if ((rc = decode_f32_pass(h, synd, batch, decoding, llr, iters, conv, second))) return rc;
    return stream_leave_histogram(h, iters, conv, batch);
}

// The float32 decode of a batch: device pointers, on h->stream; `llr` receives FP64 values, each an FP32 posterior widened.
int decode_f32(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    int rc;
    if ((rc = decode_gate(h, h->row_probs ? "per-row channel probabilities are" : nullptr, false))) return rc;  // (the entry points have said so already)
    // Small codes stay on chip where plan_f32_route (host_onchip.h) says so -- one launch, messages in registers (the lane = edge families) or, with
    // ldpc_hip_bp_set_f32_lane_node on, in LDS (the lane = node kernel).  Its answer is 0 under small_mode 0 and 2, the switch F32_ONCHIP 0, and any
    // switch that names the per-pass kernels below (F32_NT, F32_GRID_ROWS, SPREAD_NODES).
    {
        bool took = false;
        rc = decode_onchip_f32(h, synd, batch, decoding, llr, iters, conv, &took);
        if (took || rc) return rc;
    }
    // A tile runs until the slowest of its 64 rows is done.  Where most rows converge early a short first pass + a second pass over the
    // compacted rest does the same work in a fraction of the tile-iterations: under the conditions of the FP64 dispatch (decode_device).
    // (switch F32_REPACK_MIN_TILES t > 0: t instead of the 512 tiles -- the tests cut batches of 70 and 200 tiles with it)
    const int64_t tiles_total = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    const int64_t min_tiles = h->sw("F32_REPACK_MIN_TILES") > 0 ? h->sw("F32_REPACK_MIN_TILES") : 512;
    if (h->repack_iters != 0 && h->max_iter >= 8 && tiles_total >= min_tiles && h->m > 0 && h->n > 0)
        return decode_f32_repacked(h, synd, batch, decoding, llr, iters, conv);
    return decode_f32_pass(h, synd, batch, decoding, llr, iters, conv, F32Pass());
}
