// host_f32.h -- host side of the float32 message mode (bp_f32_kernels.h): what it refuses, its workspace, a chunk's rounds queued
// Part of libldpc_hip.so: included by tu_f32.hip.  Modelled on the per-pass route of host_stream.h (StreamPlan::rp): per-pass kernels
// from the first iteration for any batch size, every round queued without waiting for the device.
#pragma once

// What the handle is set up for that the float32 mode cannot do; *what: the caller's own addition (row priors, soft syndromes) or nullptr.
int f32_refusal(const ldpc_hip_bp *h, const char *what) {
    if (h->msg_dtype != LDPC_HIP_MSG_F32) return LDPC_HIP_OK;
    if (what) return fail(LDPC_HIP_ERR_UNSUPPORTED, "float32 messages: %s not available (set the message dtype to float64)", what);
    if (h->bp_method != LDPC_HIP_MINIMUM_SUM)
        return fail(LDPC_HIP_ERR_UNSUPPORTED, "float32 messages: product-sum is not available (its tanh / log have no bit-exact FP32 form here); use minimum-sum or float64");
    if (h->schedule != 1 || h->random_serial)
        return fail(LDPC_HIP_ERR_UNSUPPORTED, "float32 messages: the serial schedules are not available (parallel schedule required)");
    return LDPC_HIP_OK;
}

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

// The float32 decode of a batch: device pointers, on h->stream; `llr` receives FP64 values, each an FP32 posterior widened.
int decode_f32(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    int rc;
    if ((rc = f32_refusal(h, h->row_probs ? "per-row channel probabilities are" : nullptr))) return rc;
    // Small codes of the lane = edge families stay on chip (host_onchip.h: decode_onchip_f32 -- one launch, messages in registers).  Off:
    // small_mode 0 (never an on-chip kernel), the switch F32_ONCHIP 0, and any switch that names the per-pass kernels below (F32_NT,
    // F32_GRID_ROWS, SPREAD_NODES: who sets one wants those kernels, on whatever code).
    if (h->small_mode != 0 && h->sw("F32_ONCHIP") != 0 && h->sw("F32_NT") < 0 && h->sw("F32_GRID_ROWS") <= 0 && h->sw("SPREAD_NODES") <= 0) {
        bool took = false;
        rc = decode_onchip_f32(h, synd, batch, decoding, llr, iters, conv, &took);
        if (took || rc) return rc;
    }
    const int64_t tiles_total = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    const size_t m1 = (size_t)(h->m ? h->m : 1), n1 = (size_t)(h->n ? h->n : 1), nnz1 = (size_t)(h->nnz ? h->nnz : 1);
    const size_t per_tile_msg = sizeof(float) * nnz1 * LDPC_WAVE, per_tile_llr = llr ? sizeof(float) * n1 * LDPC_WAVE : 0;
    int64_t chunk = 0;
    if ((rc = chunk_tiles_that_fit(h, tiles_total, f32_tile_bytes(h, llr != nullptr), h->msgA.cap + h->msgC.cap + h->llr_t.cap, 0.85, 32768, "syndrome", &chunk))) return rc;
    const size_t ct = (size_t)chunk;
    // (nzm: no float32 kernel reads it -- min-sum needs the parity word and the invalid mask only; it exists because pack_syndromes_kernel writes it)
    if ((rc = h->msgA.ensure(per_tile_msg * ct)) || (rc = h->msgC.ensure(per_tile_msg * ct))) return rc;
    if ((rc = h->par.ensure(sizeof(uint64_t) * m1 * ct)) || (rc = h->nzm.ensure(sizeof(uint64_t) * m1 * ct)) || (rc = h->invalid.ensure(sizeof(uint64_t) * ct))) return rc;
    if ((rc = h->dec.ensure(sizeof(uint64_t) * n1 * ct)) || (rc = h->dcur.ensure(sizeof(uint64_t) * n1 * ct))) return rc;
    if (per_tile_llr && (rc = h->llr_t.ensure(per_tile_llr * ct))) return rc;
    if ((rc = h->tile_state.ensure(sizeof(TileState) * ct)) || (rc = h->handoff_list.ensure(sizeof(int32_t) * ct)) || (rc = h->counter.ensure(16))) return rc;
    if ((rc = h->f32_llr0.ensure(sizeof(float) * n1))) return rc;
    reset_timing(h, false);
    hipStream_t st = h->stream;
    if (h->n > 0) LDPC_LAUNCH(bp_f32_priors_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, st, (const double *)h->d_llr0, h->n, (float *)h->f32_llr0.p);
    HIPCHK(hipGetLastError());
    for (int64_t t0 = 0; t0 < tiles_total; t0 += chunk) {
        const ChunkRange c = chunk_range(t0, chunk, tiles_total, batch);
        const unsigned tiles = (unsigned)c.tiles;
        HIPCHK(hipMemsetAsync(h->invalid.p, 0, sizeof(uint64_t) * (size_t)c.tiles, st));
        HIPCHK(hipMemsetAsync(h->dec.p, 0, sizeof(uint64_t) * n1 * (size_t)c.tiles, st));
        HIPCHK(hipMemsetAsync(h->counter.p, 0, 16, st));
        if (h->m > 0)
            LDPC_LAUNCH(pack_syndromes_kernel, dim3((unsigned)((h->m + 255) / 256), tiles), dim3(256), 0, st, synd + c.b0 * h->m, c.nb, h->m,
                               (uint64_t *)h->par.p, (uint64_t *)h->nzm.p, (uint64_t *)h->invalid.p, (const int32_t *)nullptr, (const unsigned *)nullptr);
        HIPCHK(hipGetLastError());
        F32Args a = {};
        a.m = h->m; a.n = h->n; a.nnz = h->nnz; a.max_iter = h->max_iter;
        a.ms_scaling_factor = h->ms_scaling_factor; a.batch = c.nb;
        a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx; a.col_ptr = h->d_col_ptr; a.csc_edge = h->d_csc_edge;
        a.llr0 = (const float *)h->f32_llr0.p;
        a.A = (float *)h->msgA.p; a.C = (float *)h->msgC.p;
        a.par = (const uint64_t *)h->par.p; a.invalid = (const uint64_t *)h->invalid.p;
        a.dec = (uint64_t *)h->dec.p; a.dcur = (uint64_t *)h->dcur.p;
        a.llr_t = per_tile_llr ? (float *)h->llr_t.p : nullptr;
        a.iters = iters ? iters + c.b0 : nullptr; a.conv = conv ? conv + c.b0 : nullptr;
        a.state = (TileState *)h->tile_state.p; a.counters = (unsigned *)h->counter.p; a.list = (int32_t *)h->handoff_list.p;
        a.host_flag = h->d_flag;
        a.seq = ++h->flag_seq ? h->flag_seq : ++h->flag_seq;  // never 0 (the word's initial value)
        // rows (columns) per wavefront, as the FP64 per-pass route chooses them (host_stream.h: stream_start_per_pass)
        a.nodes = h->sw("SPREAD_NODES") > 0 ? h->sw("SPREAD_NODES") : tiles <= 8 ? 1 : tiles < 512 ? 4 : 16;
        if ((rc = chunk_timing_begin(h))) return rc;
        LDPC_LAUNCH(bp_f32_state_init_kernel, dim3((tiles + 255) / 256), dim3(256), 0, st, a, (int)tiles);
        LDPC_LAUNCH(bp_f32_init_kernel, dim3((unsigned)(h->nnz ? (h->nnz + 63) / 64 : 1), tiles), dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        // Every kernel of a round loops over the listed tiles, so a launch needs only enough workgroup rows to fill the chip: all the
        // tiles while they are few, else what gives ~16 384 workgroups (at least 256 rows).  Once tiles have finished the list is
        // compacted every 4 rounds and the rows beyond it leave at once.
        // (switch F32_GRID_ROWS k > 0: at most k rows for all four kernels -- the tests reach gridDim.y < count at 70 tiles with it)
        const int grid_rows = h->sw("F32_GRID_ROWS");
        auto rows_for = [&](unsigned gx) {
            const unsigned want = grid_rows > 0 ? (unsigned)grid_rows : 16384u / gx > 256u ? 16384u / gx : 256u;
            return tiles < want ? tiles : want;
        };
        const unsigned per_wg = 4u * (unsigned)a.nodes;
        const unsigned gcx = (unsigned)(h->m ? (h->m + per_wg - 1) / per_wg : 1), gbx = (unsigned)(h->n ? (h->n + per_wg - 1) / per_wg : 1);
        const unsigned gsx = (unsigned)(h->m ? (h->m + 255) / 256 : 1), gfx = (unsigned)(h->n ? (h->n + 63) / 64 : 1);
        // messages of the tiles in flight beyond ~the MALL are streamed, not cached (as stream_rounds decides it)
        // (switch F32_NT 0 / 1: the policy whatever the size -- the tests run the non-temporal instantiations on a small case with it)
        const bool nt = h->sw("F32_NT") >= 0 ? h->sw("F32_NT") > 0 : (double)tiles * 2.0 * (double)per_tile_msg > 384.0 * 1024.0 * 1024.0;
        const F32Kernels k = pick_f32(h, nt);
        const volatile unsigned *flag = h->h_flag;
        for (int round = 0; round < h->max_iter; ++round) {
            if (*flag == a.seq) break;  // a look, not a wait: the device has reported the last tile final
            a.round = round;
            if (round >= 4 && round % 4 == 0) LDPC_LAUNCH(bp_f32_compact_kernel, dim3(1), dim3(64), 0, st, a);
            LDPC_LAUNCH(k.check, dim3(gcx, rows_for(gcx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(k.bit, dim3(gbx, rows_for(gbx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(bp_f32_synd_kernel, dim3(gsx, rows_for(gsx)), dim3(256), 0, st, a);
            LDPC_LAUNCH(bp_f32_finish_kernel, dim3(gfx, rows_for(gfx)), dim3(256), 0, st, a);
        }
        HIPCHK(hipGetLastError());
        if ((rc = chunk_timing_end(h))) return rc;
        if (h->n > 0) {
            LDPC_LAUNCH(unpack_decoding_kernel, dim3((unsigned)((h->n + 255) / 256), tiles), dim3(256), 0, st, (const uint64_t *)h->dec.p, c.nb, h->n,
                               decoding + c.b0 * h->n, (const int32_t *)nullptr, (const unsigned *)nullptr);
            if (llr)
                LDPC_LAUNCH(bp_f32_transpose_llr_kernel, dim3((unsigned)((h->n + LDPC_WAVE - 1) / LDPC_WAVE), tiles), dim3(256), 0, st,
                                   (const float *)h->llr_t.p, c.nb, h->n, llr + (size_t)c.b0 * h->n);
        }
        HIPCHK(hipGetLastError());
    }
    return LDPC_HIP_OK;
}
