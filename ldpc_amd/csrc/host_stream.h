// host_stream.h -- host side of the streamed kernels: a pass planned and queued (plan_stream, decode_streamed), the dispatch (decode_device), the two-pass decode
// Part of libldpc_hip.so: included by bp_hip.hip (one translation unit), in the order given there.
#pragma once

// The per-pass kernels of a round.  nt: non-temporal cache policy for the message traffic (tiles that outgrow the 256 MB MALL; see MsgBufT).
// The LOOP forms serve the slots beyond the first 32 of a compacted list.  rp: every lane's own prior (row priors: SpreadArgs::llr0_t) in the
// bit and finish kernels; no LOOP forms -- such a decode is never a compacted second pass.
struct SpreadKernels { spread_kernel_t check = nullptr, bit = nullptr, check_loop = nullptr, bit_loop = nullptr, finish = nullptr; };
static SpreadKernels pick_spread(const ldpc_hip_bp *h, bool nt, bool rp, bool mem) {
    SpreadKernels k;
    const int dr = h->max_row_deg, dc = h->max_col_deg;
    if (mem) {  // memory min-sum (decode_gate: minimum-sum only); no LOOP forms either -- such a decode is not cut in two passes
        pick_spread_mem(dr, dc, nt, k.check, k.bit);
        k.finish = bp_spread_mem_finish_kernel;
        return k;
    }
    if (rp) with_method_math(h, [&](auto M, auto F) { pick_spread_m<M, F, false, true>(dr, dc, nt, k.check, k.bit); });
    else {
        with_method_math(h, [&](auto M, auto F) { pick_spread_m<M, F, false>(dr, dc, nt, k.check, k.bit); });
        with_method_math(h, [&](auto M, auto F) { pick_spread_m<M, F, true>(dr, dc, nt, k.check_loop, k.bit_loop); });
    }
    k.finish = rp ? bp_spread_finish_kernel<false, true> : bp_spread_finish_kernel<false>;
    return k;
}

// Item tables of the variable-degree ring (bp_stream_kernel.h, LDPC_RING_VAR): the check rows, and the pairs of bit columns, in the
// order the wavefronts take them -- wavefront w of a workgroup of W takes entries w, w + W, w + 2 W, ...  Blocks of W items come
// alternately from the heavy and from the light end of the items sorted by size, so that along a wavefront's sequence a heavy item
// is followed by a light one and two consecutive items fit its queue together.  (The order changes nothing in the results: the rows
// of a check pass, and the columns of a bit pass, are independent of each other.)
static int ensure_var_ring_items(ldpc_hip_bp *h, int W) {
    if (h->var_items_built) return 0;
    const int m = h->m, n = h->n, pairs = (n + 1) / 2;
    std::vector<int32_t> col_ptr((size_t)n + 1, 0);
    for (int32_t c : h->h_col_idx) ++col_ptr[(size_t)c + 1];
    for (int j = 0; j < n; ++j) col_ptr[(size_t)j + 1] += col_ptr[(size_t)j];
    auto interleave = [W](std::vector<std::array<int32_t, 4>> &items) {
        auto units = [](const std::array<int32_t, 4> &it) { return (it[2] + (it[3] > 0 ? it[3] : 0) + 1) / 2; };
        std::stable_sort(items.begin(), items.end(), [&](const std::array<int32_t, 4> &x, const std::array<int32_t, 4> &y) { return units(x) > units(y); });
        std::vector<std::array<int32_t, 4>> out;
        out.reserve(items.size());
        size_t lo = 0, hi = items.size();
        for (bool heavy = true; lo < hi; heavy = !heavy)
            for (int k = 0; k < W && lo < hi; ++k) out.push_back(heavy ? items[lo++] : items[--hi]);
        items.swap(out);
    };
    std::vector<std::array<int32_t, 4>> rows((size_t)m), prs((size_t)pairs);
    for (int i = 0; i < m; ++i) rows[(size_t)i] = {h->h_row_ptr[(size_t)i], i, h->h_row_ptr[(size_t)i + 1] - h->h_row_ptr[(size_t)i], 0};
    for (int g = 0; g < pairs; ++g) {
        const int j0 = 2 * g, j1 = j0 + 1;
        prs[(size_t)g] = {col_ptr[(size_t)j0], g, col_ptr[(size_t)j0 + 1] - col_ptr[(size_t)j0], j1 < n ? col_ptr[(size_t)j1 + 1] - col_ptr[(size_t)j1] : -1};
    }
    interleave(rows);
    interleave(prs);
    int rc;
    if ((rc = h->var_row_items.ensure(16 * (size_t)(m ? m : 1)))) return rc;
    if ((rc = h->var_pair_items.ensure(16 * (size_t)(pairs ? pairs : 1)))) return rc;
    if (m) HIPCHK(hipMemcpy(h->var_row_items.p, rows.data(), 16 * (size_t)m, hipMemcpyHostToDevice));
    if (pairs) HIPCHK(hipMemcpy(h->var_pair_items.p, prs.data(), 16 * (size_t)pairs, hipMemcpyHostToDevice));
    h->var_items_built = true;
    return 0;
}

// ---- the streamed decode: one pass of the flooding schedule over the batch, chunk by chunk ------------------------------------------------
// Everything below runs on h->stream with device pointers only.

// What a pass is told.  Default: a plain decode to h->max_iter.  decode_stream_repacked builds a first pass that stops early and leaves its messages
// behind, and the continuation that carries on the rows it left: known to the device only -- `batch` is the most there can be, the kernels read the
// real count (rows_dev) and reach the caller's rows through row_map; the grids of its tile-looping kernels follow an estimate.
struct StreamPass {
    int max_iter = -1;                    // iteration limit of this pass (-1: the handle's)
    bool keep_state = false;              // a first pass: its last bit pass must leave the messages behind (BpArgs::keep_state)
    double *A = nullptr, *C = nullptr;    // continuation: its bit_to_check (compacted here, from C) / check_to_bit arrays
    int32_t it_start = 0;                 // ... iterations its rows have behind them
    const int32_t *row_map = nullptr;     // ... its rows in the caller's arrays (BpArgs::row_map)
    const unsigned *rows_dev = nullptr;   // ... {rows, tiles} on the device (BpArgs::rows_dev)
    int64_t grid_tiles = 0;               // ... grid.y of its tile-looping kernels (an estimate; they loop)
    int64_t late_rows = -1;               // ... rows the steering histogram expects to be still running 8 iterations into it (-1: unknown)
    const double *relay_ag = nullptr;     // a leg of Relay-BP (decode_relay): a[] and gamma[] of the leg, [2][n] -- a memory decode with them, to max_iter
    const double *relay_seed = nullptr;   // ... after the first: the previous leg's posteriors [batch][n], what M and the initial messages start from
    bool continues() const { return A != nullptr; }
};

// Tiles per chunk of a streamed decode of tiles_total tiles.  A tile holds both message arrays, the log-ratios if wanted, the packed syndromes and
// decisions, its own priors under row priors (rp); 32768: grid.y of the pack / unpack launches stays below 65536
static int stream_chunk_tiles(const ldpc_hip_bp *h, int64_t tiles_total, bool want_llr, bool rp, int64_t *chunk) {
    const size_t per_tile_msg = sizeof(double) * (size_t)(h->nnz ? h->nnz : 1) * LDPC_WAVE, per_tile_n = sizeof(double) * (size_t)(h->n ? h->n : 1) * LDPC_WAVE;
    const size_t per_tile = 2 * per_tile_msg + (want_llr ? per_tile_n : 0) + 16 * (size_t)(h->m + h->n + 1) + (rp ? sizeof(double) * (size_t)h->n * LDPC_WAVE : 0);
    return chunk_tiles_that_fit(h, tiles_total, per_tile, h->msgA.cap + h->msgC.cap + h->llr_t.cap, 0.85, 32768, "syndrome", chunk);
}

// What a pass decides once, before its first chunk.
struct StreamPlan {
    int max_iter = 0;     // the pass's iteration limit
    bool mem = false;     // memory min-sum (h->variant): as rp -- the per-pass kernels from the first iteration, bp_spread_mem_*; M lives where the row priors would
    bool rp = false;      // row priors (h->row_probs [batch][n]): the per-pass kernels from the first iteration whatever the batch size -- no persistent kernel, no edge0, no hand-off
    int64_t chunk = 0;    // tiles per chunk
    size_t per_tile_msg = 0, per_tile_llr = 0;  // bytes of one message array / of the log-ratios (0: not wanted) per tile
    KernelChoice kern = {};                     // the persistent kernel
    int var_units = 0;                          // ... variable-degree ring: 1 KiB units of LDS per wavefront
    size_t lds_per_wave = 0;                    // ... dynamic LDS per wavefront
    int handoff = 0;                            // tiles the persistent kernel parks for the per-pass kernels; a chunk of no more starts per-pass
};

static int plan_stream(const ldpc_hip_bp *h, int64_t tiles_total, bool want_llr, const StreamPass &pass, StreamPlan &p) {
    p.max_iter = pass.max_iter < 0 ? h->max_iter : pass.max_iter;
    p.rp = h->row_probs != nullptr;
    p.mem = h->variant == Variant::Memory || pass.relay_ag != nullptr;
    p.per_tile_msg = sizeof(double) * (size_t)(h->nnz ? h->nnz : 1) * LDPC_WAVE;
    p.per_tile_llr = want_llr ? sizeof(double) * (size_t)(h->n ? h->n : 1) * LDPC_WAVE : 0;
    int rc;
    if ((rc = stream_chunk_tiles(h, tiles_total, want_llr, p.rp || p.mem, &p.chunk))) return rc;
    if (pass.continues() && p.chunk < tiles_total) return fail(LDPC_HIP_ERR_NOMEM, "internal: the second pass of a compacted decode must be one chunk");
    const int ring = h->regular ? h->ring_depth : 0;
    // the variable-degree ring (bp_stream_kernel.h, LDPC_RING_VAR) on request (VAR_RING 1) wherever it applies -- rows <= 16, columns <= 8.
    // Measured on the irregular n = 10 000 code (profiles/r5_irregular_paths.txt): +5 % over the register variant for product-sum, -4 % for
    // min-sum, and below the per-pass kernels for product-sum -- so it is not what runs by default anywhere.
    const bool var_ring = h->m > 0 && h->n > 0 && h->max_row_deg <= 16 && h->max_col_deg <= 8 && h->on("VAR_RING");
    p.kern = with_method_math(h, [&](auto M, auto F) { return pick_kernel<M, F>(h->max_row_deg, h->max_col_deg, ring, var_ring); });
    p.var_units = !p.kern.var_ring ? 0 : h->sw("VAR_RING_UNITS") >= 8 ? (h->sw("VAR_RING_UNITS") <= 40 ? h->sw("VAR_RING_UNITS") : 40) : 11;
    // ring variant: each wavefront owns RING slots of dynamic LDS + the parking space of the exact product-sum check row (LDPC_NEAR_BYTES, behind the rings)
    const size_t near_bytes = (h->bp_method == LDPC_HIP_PRODUCT_SUM && h->math_mode == LDPC_HIP_MATH_LIBM_EXACT) ? LDPC_NEAR_BYTES : 0;
    p.lds_per_wave = (p.kern.var_ring ? (size_t)p.var_units * 1024u : (size_t)p.kern.ring_slot_bytes * (size_t)p.kern.ring_depth) + near_bytes;
    // Product-sum on a matrix without a fixed-degree ring variant (irregular, or regular of another shape than (6,3) / (8,4), or the ring
    // switched off): the persistent kernel holds the check pass AND the bit pass in one register allocation -- 128 VGPRs with rows of up to 6
    // entries, 158-168 with 8 or 16: four, then three wavefronts per SIMD -- while the per-pass kernels hold one pass each (73-106 and 46-62
    // VGPRs: 4-6 and 8 per SIMD), and the exact product-sum arithmetic is a dependent chain per wavefront that needs the wavefronts: they get
    // through the same tile-iterations in 0.64 of the cycles (counter pass in profiles/r5_irregular_paths.txt).  So unless the caller set a
    // threshold such a batch takes the per-pass kernels from its first iteration: 0.45 -> 0.56 of HBM on the irregular code with rows of 3 .. 16
    // entries, 0.49 -> 0.63 and 0.46 -> 0.59 with rows of 3 .. 8, 0.57 -> 0.60 on the headline code with its ring off.  Min-sum has no such
    // chain and stays with the persistent kernel (0.69-0.77 against 0.65-0.68), and so do the ring variants (80 VGPRs: 0.65 against 0.60).
    // Bounded: a per-pass round is four launches over EVERY tile of the chunk (a row of workgroups per tile, leaving at once when the tile is
    // final: ~50 us per 256 rows and launch), queued by the host until the device reports the last tile final.  With one hopeless syndrome
    // and the reference's default max_iter = n that is thousands of full-size, empty rounds -- a cost that grows with the batch.  So only
    // decodes of at most 128 iterations start per-pass; longer ones keep the persistent kernel, whose hand-off parks at most 256 tiles
    // (the cost of an empty round is then the fixed ~0.2 ms it always was).
    const bool per_pass_first = h->handoff < 0 && h->bp_method == LDPC_HIP_PRODUCT_SUM && p.kern.ring_depth == 0 && !p.kern.var_ring &&
                                h->max_row_deg <= 16 && h->max_col_deg <= 8 && p.max_iter <= 128;
    p.handoff = h->handoff < 0 ? (per_pass_first ? INT32_MAX : 256) : h->handoff;
    return LDPC_HIP_OK;
}

// Wavefronts per workgroup of the persistent kernel (one workgroup = one 64-syndrome tile).  Register variant: 128 VGPRs,
// 16 wavefronts per CU -> 4-wave workgroups once there are >= 4 tiles per CU.  Ring variant:
// ~70 VGPRs and 6 KiB of LDS per wavefront -> 24 wavefronts per CU as two 12-wave workgroups
// (3 wavefronts on each SIMD; measured best on MI355X, profiles/; 6-wave workgroups place
// unevenly on the 4 SIMDs and 8-wave ones leave a ragged last round at 1024 tiles).
static int stream_waves(const ldpc_hip_bp *h, const StreamPlan &p, int64_t tiles) {
    int waves = h->waves_per_wg;
    if (waves <= 0) {
        if (p.kern.ring_depth) waves = tiles >= 512 ? 12 : 16;
        else if (p.kern.var_ring) waves = p.kern.max_waves;
        else waves = tiles >= 1024 ? 4 : (tiles >= 512 ? 8 : 16);
    }
    if (waves > p.kern.max_waves) waves = p.kern.max_waves;
    while (p.lds_per_wave * (size_t)waves > 144u * 1024u) --waves;  // stay below the 160 KiB of a CU
    return waves;
}

// the workspace of a chunk's tiles
static int stream_workspace(ldpc_hip_bp *h, const StreamPlan &p) {
    const size_t m1 = (size_t)(h->m ? h->m : 1), n1 = (size_t)(h->n ? h->n : 1), chunk = (size_t)p.chunk;
    int rc;
    if ((rc = h->msgA.ensure(p.per_tile_msg * chunk)) || (rc = h->msgC.ensure(p.per_tile_msg * chunk))) return rc;
    if ((rc = h->par.ensure(sizeof(uint64_t) * m1 * chunk)) || (rc = h->nzm.ensure(sizeof(uint64_t) * m1 * chunk)) || (rc = h->invalid.ensure(sizeof(uint64_t) * chunk))) return rc;
    if ((rc = h->dec.ensure(sizeof(uint64_t) * n1 * chunk)) || (rc = h->dcur.ensure(sizeof(uint64_t) * n1 * chunk))) return rc;
    if (p.per_tile_llr && (rc = h->llr_t.ensure(p.per_tile_llr * chunk))) return rc;
    if ((p.rp || p.mem) && (rc = h->rowp_llr.ensure(sizeof(double) * n1 * LDPC_WAVE * chunk))) return rc;  // (per chunk, like the messages; memory: M)
    if ((rc = h->tile_state.ensure(sizeof(TileState) * chunk)) || (rc = h->handoff_list.ensure(sizeof(int32_t) * chunk)) || (rc = h->counter.ensure(16))) return rc;
    if (!h->h_counters) HIPCHK(hipHostMalloc((void **)&h->h_counters, 16, hipHostMallocDefault));
    return LDPC_HIP_OK;
}

// a chunk's syndromes, bit-packed by tile (loop_tiles: grid.y of the kernels that loop over tiles -- a continuation's estimate, else the chunk's tiles)
static int stream_pack(ldpc_hip_bp *h, const StreamPass &pass, const ChunkRange &c, unsigned loop_tiles, const uint8_t *synd) {
    HIPCHK(hipMemsetAsync(h->invalid.p, 0, sizeof(uint64_t) * (size_t)c.tiles, h->stream));
    HIPCHK(hipMemsetAsync(h->dec.p, 0, sizeof(uint64_t) * (size_t)(h->n ? h->n : 1) * (size_t)c.tiles, h->stream));
    if (h->m > 0) {
        dim3 g((unsigned)((h->m + 255) / 256), loop_tiles);
        LDPC_LAUNCH(pack_syndromes_kernel, g, dim3(256), 0, h->stream, synd + c.b0 * h->m, c.nb, h->m, (uint64_t *)h->par.p, (uint64_t *)h->nzm.p, (uint64_t *)h->invalid.p, pass.row_map, pass.rows_dev);
    }
    return LDPC_HIP_OK;
}
static BpArgs stream_bp_args(const ldpc_hip_bp *h, const StreamPlan &p, const StreamPass &pass, const ChunkRange &c, int32_t *iters, uint8_t *conv) {
    BpArgs a = {};
    a.m = h->m; a.n = h->n; a.nnz = h->nnz; a.max_iter = p.max_iter;
    a.ms_scaling_factor = h->ms_scaling_factor; a.batch = c.nb; a.llr0 = h->d_llr0;
    a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx; a.col_ptr = h->d_col_ptr; a.csc_edge = h->d_csc_edge;
    a.A = (double *)h->msgA.p; a.C = (double *)h->msgC.p;
    if (pass.continues()) { a.A = pass.A; a.C = pass.C; a.it_start = pass.it_start; a.rows_dev = pass.rows_dev; a.row_map = pass.row_map; }
    a.keep_state = pass.keep_state ? 1 : 0;
    a.par = (const uint64_t *)h->par.p; a.nzm = (const uint64_t *)h->nzm.p; a.invalid = (const uint64_t *)h->invalid.p;
    a.dec = (uint64_t *)h->dec.p; a.dcur = (uint64_t *)h->dcur.p;
    a.llr_t = p.per_tile_llr ? (double *)h->llr_t.p : nullptr;
    a.iters = iters ? iters + c.b0 : nullptr; a.conv = conv ? conv + c.b0 : nullptr;
    a.state = (TileState *)h->tile_state.p; a.counters = (unsigned *)h->counter.p; a.handoff_list = (int32_t *)h->handoff_list.p;
    a.total_tiles = (int32_t)c.tiles; a.handoff_threshold = p.handoff; a.clk = h->d_clk;
    if (p.kern.var_ring) { a.row_items = (const int32_t *)h->var_row_items.p; a.pair_items = (const int32_t *)h->var_pair_items.p; a.ring_units = p.var_units; }
    return a;
}

// The per-pass rounds a chunk queues: `grid_tiles` workgroup rows (0: none), at most `rounds` rounds.  How many of the rows have a tile is known to the
// host only when the chunk skips the persistent kernel (sa.n_tiles >= 0), otherwise the kernels read it from counters[1].
struct SpreadRounds { unsigned grid_tiles = 0; int rounds = 0; };

// per-pass launches from the start: so few tiles that they would each sit on one compute unit (tiles <= handoff; per_pass_first: any number), or row priors
static int stream_start_per_pass(ldpc_hip_bp *h, const StreamPlan &p, int64_t tiles, SpreadArgs &sa, SpreadRounds &r) {
    r.grid_tiles = (unsigned)tiles;
    r.rounds = p.max_iter - sa.bp.it_start;
    sa.n_tiles = (int32_t)tiles;
    // rows (columns) per wavefront of a per-pass workgroup: 1 when a handful of tiles must fill the chip, 4 up to a few hundred
    // tiles (the chunks of the pipelined host path among them), 16 from 512 on -- a workgroup's start (the logarithm table into
    // LDS, the tile's state) is then paid per 64 rows instead of per 16: 0.563 against 0.535 of HBM on the irregular code's 512
    // tiles, same box (profiles/r5_irregular_paths.txt)
    sa.nodes = h->sw("SPREAD_NODES") > 0 ? h->sw("SPREAD_NODES") : tiles <= 8 ? 1 : tiles < 512 ? 4 : 16;
    LDPC_LAUNCH(bp_spread_state_init_kernel, dim3((r.grid_tiles + 255) / 256), dim3(256), 0, h->stream, sa);
    const dim3 gi((unsigned)(h->nnz ? (h->nnz + 63) / 64 : 1), r.grid_tiles);  // (a grid dimension must not be 0: empty matrices)
    if (p.mem && sa.relay_seed)
        LDPC_LAUNCH(bp_spread_relay_init_kernel, gi, dim3(256), 0, h->stream, sa);
    else if (p.mem)
        LDPC_LAUNCH(bp_spread_mem_init_kernel, gi, dim3(256), 0, h->stream, sa);
    else if (p.rp)
        with_method_math(h, [&](auto M, auto F) { LDPC_LAUNCH((bp_spread_init_kernel<M, F, true>), gi, dim3(256), 0, h->stream, sa); });
    else if (sa.bp.it_start == 0)  // (else the message state is there already)
        with_method_math(h, [&](auto M, auto F) { LDPC_LAUNCH((bp_spread_init_kernel<M, F>), gi, dim3(256), 0, h->stream, sa); });
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}
// the persistent kernel, a workgroup per tile; with a hand-off it parks its last tiles for the per-pass rounds (a parked tile has completed >= 1
// iteration and knows its own it0)
static int stream_persistent(ldpc_hip_bp *h, const StreamPlan &p, int64_t tiles, int waves, BpArgs a, SpreadArgs &sa, SpreadRounds &r) {
    int rc;
    if (p.kern.ring_depth && h->n > 0 && !h->on("EXPLICIT_INIT")) {  // the first check pass reads this table instead of initial messages
        if ((rc = h->d_edge0.ensure(sizeof(double) * (size_t)h->n))) return rc;
        const dim3 ge((unsigned)((h->n + 255) / 256));
        with_method_math(h, [&](auto M, auto F) { LDPC_LAUNCH((bp_edge0_kernel<M, F>), ge, dim3(256), 0, h->stream, h->d_llr0, h->n, (double *)h->d_edge0.p); });
        a.edge0 = (const double *)h->d_edge0.p;
    }
    LDPC_LAUNCH(p.kern.fn, dim3((unsigned)tiles), dim3((unsigned)(waves * LDPC_WAVE)), (unsigned)(p.lds_per_wave * (size_t)waves), h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_mid, h->stream));
    h->timed_mid = true;
    if (p.handoff > 0 && p.max_iter > 1) {
        // the persistent kernel parks at most `handoff` tiles (it starts parking when that many are unfinished);
        // how many it did park stays on the device
        r.grid_tiles = (unsigned)(tiles < p.handoff ? tiles : p.handoff);
        r.rounds = p.max_iter - 1;
        sa.n_tiles = -1;
        sa.nodes = 4;  // (4, 8 and 16 measure the same on the headline's last 256 tiles)
    }
    return LDPC_HIP_OK;
}

// Finish the tiles with chip-wide per-pass launches: check, bit, syndrome test, bookkeeping.  Every
// round is queued at once; the host never waits.  A tile that is final (or a workgroup row without a tile)
// leaves each kernel at its first instruction, and once the device has reported "nothing left" through
// the host-mapped flag the host stops queueing -- which only matters when max_iter is far larger than
// the iterations needed (the reference's default max_iter = n).
static int stream_rounds(ldpc_hip_bp *h, const StreamPlan &p, const StreamPass &pass, SpreadArgs sa, const SpreadRounds &r) {
    hipStream_t st = h->stream;
    const unsigned grid_tiles = r.grid_tiles;
    // messages of the tiles in flight: 2 arrays x nnz x 512 B each; beyond ~the MALL they are streamed, not cached
    // (switch SPREAD_NT 0 / 1: the policy whatever the size -- the tests run the non-temporal instantiations on a small case with it)
    const bool nt = h->sw("SPREAD_NT") >= 0 ? h->sw("SPREAD_NT") > 0 : (double)grid_tiles * 2.0 * (double)p.per_tile_msg > 384.0 * 1024.0 * 1024.0;
    const SpreadKernels k = pick_spread(h, nt, p.rp, p.mem);
    const unsigned per_wg = 4u * (unsigned)sa.nodes;
    const dim3 gc((unsigned)(h->m ? (h->m + per_wg - 1) / per_wg : 1), grid_tiles), gb((unsigned)(h->n ? (h->n + per_wg - 1) / per_wg : 1), grid_tiles);
    const dim3 gs((unsigned)(h->m ? (h->m + 255) / 256 : 1), grid_tiles), gf((unsigned)(h->n ? (h->n + 63) / 64 : 1), grid_tiles);
    const volatile unsigned *flag = h->h_flag;
    // Late rounds (bp_spread_kernels.h): where the steering histogram of a two-pass decode shows at most 24 rows still running 8
    // iterations into the second pass, its list of tiles is compacted on the device every 8 rounds and a round becomes 32 rows of
    // workgroups for the list's first 32 slots + 8 rows of the looping form for whatever lies beyond (normally nothing), instead of
    // `grid_tiles` rows that leave at once at ~50 us a launch.  Not elsewhere: when most tiles keep going (the headline's last 256
    // tiles run to iteration 50, a chunk of the pipelined host path likewise) the row-per-tile grid is what runs them fastest.
    const bool may_compact = pass.rows_dev != nullptr && pass.late_rows >= 0 && pass.late_rows <= 24 && grid_tiles > 40;
    bool compacted = false;
    for (int round = 0; round < r.rounds; ++round) {
        if (*flag == sa.seq) break;  // a look, not a wait
        sa.round = round;
        sa.slot0 = 0;
        if (may_compact && round >= 8 && round % 8 == 0) {
            LDPC_LAUNCH(bp_spread_compact_kernel, dim3(1), dim3(64), 0, st, sa);
            sa.n_tiles = -1;  // (the count is the device's from here on: counters[1])
            compacted = true;
        }
        if (!compacted) {
            LDPC_LAUNCH(k.check, gc, dim3(256), 0, st, sa);
            LDPC_LAUNCH(k.bit, gb, dim3(256), 0, st, sa);
            LDPC_LAUNCH(bp_spread_synd_kernel<false>, gs, dim3(256), 0, st, sa);
            LDPC_LAUNCH(k.finish, gf, dim3(256), 0, st, sa);
        } else {
            SpreadArgs sb = sa;
            sb.slot0 = 32;
            LDPC_LAUNCH(k.check, dim3(gc.x, 32), dim3(256), 0, st, sa);
            LDPC_LAUNCH(k.check_loop, dim3(gc.x, 8), dim3(256), 0, st, sb);
            LDPC_LAUNCH(k.bit, dim3(gb.x, 32), dim3(256), 0, st, sa);
            LDPC_LAUNCH(k.bit_loop, dim3(gb.x, 8), dim3(256), 0, st, sb);
            LDPC_LAUNCH(bp_spread_synd_kernel<false>, dim3(gs.x, 32), dim3(256), 0, st, sa);
            LDPC_LAUNCH(bp_spread_synd_kernel<true>, dim3(gs.x, 8), dim3(256), 0, st, sb);
            LDPC_LAUNCH(k.finish, dim3(gf.x, 32), dim3(256), 0, st, sa);
            LDPC_LAUNCH(bp_spread_finish_kernel<true>, dim3(gf.x, 8), dim3(256), 0, st, sb);
        }
    }
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// a chunk's packed decisions (h->dec) and tile-major log-ratios (h->llr_t) into the caller's arrays (a continuation: through its row map)
static int stream_outputs(ldpc_hip_bp *h, const StreamPass &pass, const ChunkRange &c, unsigned loop_tiles, uint8_t *decoding, double *llr) {
    if (h->n > 0) {
        dim3 g((unsigned)((h->n + 255) / 256), loop_tiles);
        LDPC_LAUNCH(unpack_decoding_kernel, g, dim3(256), 0, h->stream, (const uint64_t *)h->dec.p, c.nb, h->n, decoding + c.b0 * h->n, pass.row_map, pass.rows_dev);
        if (llr) {
            dim3 gt((unsigned)((h->n + LDPC_WAVE - 1) / LDPC_WAVE), loop_tiles);
            LDPC_LAUNCH(transpose_llr_kernel, gt, dim3(256), 0, h->stream, (const double *)h->llr_t.p, c.nb, h->n, llr + (size_t)c.b0 * h->n, pass.row_map, pass.rows_dev);
        }
    }
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// One pass over the batch.  *chunk_tiles (if asked for): the tiles per chunk it used (== tiles_total: the whole batch's state is resident).
static int decode_streamed(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv,
                           const StreamPass &pass, int64_t *chunk_tiles = nullptr) {
    const int64_t tiles_total = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    StreamPlan p;
    int rc;
    if ((rc = plan_stream(h, tiles_total, llr != nullptr, pass, p)) || (rc = stream_workspace(h, p))) return rc;
    if (chunk_tiles) *chunk_tiles = p.chunk;
    if (p.kern.var_ring && (rc = ensure_var_ring_items(h, p.kern.max_waves))) return rc;
    reset_timing(h, false);  // (a second pass keeps the first pass's events, timed_prev: ldpc_hip_bp_last_kernel_ms adds them)
    hipStream_t st = h->stream;
    for (int64_t t0 = 0; t0 < tiles_total; t0 += p.chunk) {
        const ChunkRange c = chunk_range(t0, p.chunk, tiles_total, batch);
        const unsigned loop_tiles = pass.rows_dev ? (unsigned)(pass.grid_tiles < c.tiles ? (pass.grid_tiles > 0 ? pass.grid_tiles : 1) : c.tiles) : (unsigned)c.tiles;
        if ((rc = stream_pack(h, pass, c, loop_tiles, synd))) return rc;
        const BpArgs a = stream_bp_args(h, p, pass, c, iters, conv);
        HIPCHK(hipMemsetAsync(h->counter.p, 0, 16, st));
        const int waves = stream_waves(h, p, c.tiles);
        if ((rc = set_dynamic_lds(p.kern.fn, p.lds_per_wave * (size_t)waves)) || (rc = chunk_timing_begin(h))) return rc;
        if (pass.continues()) {
            // the listed rows' message state after the first pass, lane by lane, into dense tiles (inside this pass's timed region)
            const int epw = 16;
            const dim3 gg((unsigned)((h->nnz + 4 * epw - 1) / (4 * epw)), loop_tiles);
            LDPC_LAUNCH(gather_lane_state_kernel, gg, dim3(256), 0, st, (const double *)pass.C, pass.row_map, (int64_t)0, h->nnz, epw, pass.A, pass.rows_dev);
            HIPCHK(hipGetLastError());
        }
        SpreadArgs sa = {};
        sa.bp = a;
        sa.host_flag = h->d_flag;
        sa.seq = ++h->flag_seq ? h->flag_seq : ++h->flag_seq;  // never 0 (the word's initial value)
        if (p.rp && h->n > 0) {  // this chunk's rows [b0, b0 + nb) of the probabilities -> priors in the layout of its tiles (inside the timed region)
            const dim3 gp((unsigned)((h->n + LDPC_WAVE - 1) / LDPC_WAVE), (unsigned)c.tiles);
            LDPC_LAUNCH(row_priors_kernel, gp, dim3(256), 0, st, h->row_probs + (size_t)c.b0 * (size_t)h->n, c.nb, h->n, (const double *)h->d_llr0, (double *)h->rowp_llr.p);
            HIPCHK(hipGetLastError());
            sa.llr0_t = (const double *)h->rowp_llr.p;
        }
        if (p.mem) {  // M of this chunk's tiles (filled by bp_spread_mem_init_kernel), a[] and gamma[]
            sa.llr0_t = (const double *)h->rowp_llr.p;
            sa.mem_ag = pass.relay_ag ? pass.relay_ag : (const double *)h->mem_ag.p;
            sa.relay_seed = pass.relay_seed ? pass.relay_seed + (size_t)c.b0 * (size_t)h->n : nullptr;
        }
        SpreadRounds r;
        const bool per_pass = p.rp || p.mem || (p.handoff > 0 && c.tiles <= p.handoff && p.max_iter - pass.it_start > 1 && !pass.rows_dev);
        if ((rc = per_pass ? stream_start_per_pass(h, p, c.tiles, sa, r) : stream_persistent(h, p, c.tiles, waves, a, sa, r))) return rc;
        if (r.grid_tiles > 0 && (rc = stream_rounds(h, p, pass, sa, r))) return rc;
        if ((rc = chunk_timing_end(h)) || (rc = stream_outputs(h, pass, c, loop_tiles, decoding, llr))) return rc;
    }
    return LDPC_HIP_OK;
}

// Two passes of the streamed parallel schedule: k1 iterations for everyone, then the rows that have not converged are
// COMPACTED: their message state is gathered, lane by lane, out of the first pass's tiles into dense tiles, and the decode
// carries on from iteration k1 + 1 on those (same operations on the same values: same results).  A 64-syndrome tile runs until
// its slowest syndrome is done and moves all 64 lanes' messages until then; after the compaction the tiles hold live lanes
// only.  (Rounds 1 - 2 restarted the gathered rows from scratch, which only pays when almost everything has converged by k1.)
// Whether and where to cut depends on the noise, which the host cannot see -- so every streamed decode leaves a histogram of
// its iteration counts behind (one tiny kernel, copied asynchronously) and the next decode on the handle prices the
// alternatives with it, in tile-iterations per tile of the batch: F(j) = fraction converged within j iterations,
//     plain        sum_j (1 - F(j-1)^64)
//     cut at k     sum_{j<=k} (1 - F(j-1)^64)  +  gather  +  (1 - F(k)) sum_{j>k} (1 - G_k(j-1)^64),  G_k = F conditioned on > k,
// gather = reading one message array of every tile and writing the live share = (1 + (1 - F(k))) * gather_cost of an iteration (the
// flooding schedule moves four arrays per iteration: 1/4; the serial schedule six segments per edge: 1/6), plus the first pass's outputs for rows that are decoded on.  No work is wasted when nothing
// converges (the first call, and every call whose predecessor says "plain", run plain); results do not depend on any of this.
// (stream_first_pass_length -- the pricing --, stream_leave_histogram and repack_rows_kernel live in host_handle.h: the float32 mode's two-pass decode,
// host_f32.h, shares them)
// Nothing here waits for the device: the second pass is queued at once, sized for the most rows there can be (all of them), and
// finds out on the device how many rows the first pass left -- osd_collect_kernel lists them, repack_rows_kernel turns the count
// into rows / tiles, every kernel of the second pass reads those (BpArgs::rows_dev) and reaches the caller's arrays through the
// list (BpArgs::row_map), so no row is copied out and back.  No extra message memory either: the compacted bit_to_check state is
// gathered into the first pass's check_to_bit array (dead by then -- every iteration starts by rewriting it) and the second
// pass uses the first pass's bit_to_check array as ITS check_to_bit array.
static int decode_stream_repacked(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    const int full = h->max_iter;
    const size_t B = (size_t)batch;
    int rc;
    if (!conv) { if ((rc = h->osd_conv.ensure(B))) return rc; conv = (uint8_t *)h->osd_conv.p; }
    if (!iters) { if ((rc = h->sp_iters.ensure(B * 4))) return rc; iters = (int32_t *)h->sp_iters.p; }
    double live = 0.5;
    StreamPass second;
    int k1 = stream_first_pass_length(h, &live, &second.late_rows, 0.25);
    const int64_t tiles1 = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    if (k1 >= 2 && k1 < full) {
        // the compaction needs the whole batch's message state resident (one chunk); else decode plainly
        int64_t chunk = 0;
        if ((rc = stream_chunk_tiles(h, tiles1, llr != nullptr, false, &chunk))) return rc;
        if (chunk < tiles1 || h->nnz == 0) k1 = 0;
    }
    if (k1 >= 2 && k1 < full) {
        StreamPass first;
        first.max_iter = k1; first.keep_state = true;
        int64_t chunk1 = 0;
        if ((rc = decode_streamed(h, synd, batch, decoding, llr, iters, conv, first, &chunk1))) return rc;
        // (else the first pass was cut into chunks after all -- free memory moved between the estimate above and its own: its message state is not
        // resident at once, so there is nothing to compact -- decode the batch plainly: same results; the first pass's work is lost)
        if (chunk1 < tiles1) k1 = 0;
    }
    if (k1 < 2 || k1 >= full) {
        if ((rc = decode_streamed(h, synd, batch, decoding, llr, iters, conv, StreamPass()))) return rc;
        return stream_leave_histogram(h, iters, conv, batch);
    }
    if ((rc = h->osd_list.ensure(B * sizeof(int32_t))) || (rc = h->osd_counters.ensure(4 * sizeof(unsigned)))) return rc;  // {count, next, rows, tiles}
    HIPCHK(hipMemsetAsync(h->osd_counters.p, 0, 4 * sizeof(unsigned), h->stream));
    LDPC_LAUNCH(osd_collect_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, conv, batch,
                       (int32_t *)h->osd_list.p, (unsigned *)h->osd_counters.p);
    LDPC_LAUNCH(repack_rows_kernel, dim3(1), dim3(1), 0, h->stream, (const unsigned *)h->osd_counters.p, (unsigned *)h->osd_counters.p + 2);
    HIPCHK(hipGetLastError());
    // the first pass's events stay readable while the second pass records its own (ldpc_hip_bp_last_kernel_ms adds both; nobody waits here)
    std::swap(h->ev0, h->evp0); std::swap(h->ev1, h->evp1); std::swap(h->ev_mid, h->evp_mid);
    h->timed_prev = h->timed; h->timed_prev_mid = h->timed_mid;
    second.A = (double *)h->msgC.p;   // compacted bit_to_check state (gathered inside decode_streamed)
    second.C = (double *)h->msgA.p;   // the gather's source, then the second pass's check_to_bit array
    second.it_start = k1; second.row_map = (const int32_t *)h->osd_list.p; second.rows_dev = (const unsigned *)h->osd_counters.p + 2;
    // grids of the tile-looping kernels: the rows the histogram expects + a margin (they loop, so any count is handled)
    second.grid_tiles = (int64_t)(live * 1.25 * (double)tiles1) + 8;
    if ((rc = decode_streamed(h, synd, batch, decoding, llr, iters, conv, second))) return rc;
    return stream_leave_histogram(h, iters, conv, batch);
}

// Relay-BP (ldpc_hip_bp_set_relay).  A code the lane = edge families or the lane = node kernel take runs all its legs in one
// launch (decode_onchip_relay: plan_relay_route).  Every other code, and every code with the on-chip kernels switched off, runs the leg loop below: leg l is a per-pass
// memory decode of the whole batch to relay_iters[l] iterations with the leg's a[] / gamma[] -- from the second leg on started from the
// posteriors the leg before it left (relay_llr, read by bp_spread_relay_init_kernel before the chunk's outputs overwrite its rows: a converged
// row's posteriors are frozen at its convergence iteration, so a leg's llr output IS the row's M at the leg's end) -- followed by
// relay_select_kernel, which keeps the lightest solution in the caller's arrays, adds up the iterations and counts the solutions.  A row that has
// its relay_stop solutions is still decoded in the later legs and the result ignored: nothing is read back, the call stays asynchronous.
// Correct everywhere, not fast: legs x iterations x four launches over every tile.
static int decode_relay(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    int rc;
    {
        bool took = false;
        rc = decode_onchip_relay(h, synd, batch, decoding, llr, iters, conv, &took);
        if (took || rc) return rc;
    }
    const size_t B = (size_t)batch, n1 = (size_t)(h->n ? h->n : 1);
    if ((rc = h->relay_dec.ensure(B * n1)) || (rc = h->relay_llr.ensure(sizeof(double) * B * n1)) || (rc = h->relay_li.ensure(sizeof(int32_t) * B)) ||
        (rc = h->relay_cv.ensure(B)) || (rc = h->relay_state.ensure(16 * B))) return rc;
    RelaySelectArgs ra = {};
    ra.batch = batch; ra.n = h->n; ra.stop_after = h->relay_stop;
    ra.llr0 = h->d_llr0;
    ra.leg_dec = (const uint8_t *)h->relay_dec.p; ra.leg_llr = (const double *)h->relay_llr.p;
    ra.leg_iters = (const int32_t *)h->relay_li.p; ra.leg_conv = (const uint8_t *)h->relay_cv.p;
    ra.best_w = (double *)h->relay_state.p;
    ra.nsol = (int32_t *)((char *)h->relay_state.p + 8 * B);
    ra.total = ra.nsol + B;
    ra.decoding = decoding; ra.llr = llr; ra.iters = iters; ra.conv = conv;
    for (int l = 0; l < h->relay_legs; ++l) {
        StreamPass leg;
        leg.max_iter = h->relay_iters[(size_t)l];
        leg.relay_ag = (const double *)h->relay_ag.p + (size_t)l * 2 * (size_t)h->n;
        leg.relay_seed = l ? (const double *)h->relay_llr.p : nullptr;
        if ((rc = decode_streamed(h, synd, batch, (uint8_t *)h->relay_dec.p, (double *)h->relay_llr.p, (int32_t *)h->relay_li.p, (uint8_t *)h->relay_cv.p, leg))) return rc;
        ra.first = l == 0; ra.last = l == h->relay_legs - 1;
        LDPC_LAUNCH(relay_select_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, h->stream, ra);
        HIPCHK(hipGetLastError());
    }
    return LDPC_HIP_OK;
}

// The dispatch of a batch to a kernel family.
int decode_device(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    const int64_t tiles_total = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
    if (tiles_total == 0) return LDPC_HIP_OK;
    h->timed_prev = h->timed_prev_mid = false;  // (what a two-pass decode before this one left)
    // Row priors (ldpc_hip_*_decode_batch_priors): every row is decoded with its own channel probabilities, h->row_probs [batch][n].  decode_onchip
    // sends them to the kernels plan_row_prior_route names (host_onchip.h: the row-prior forms of the lane = edge and lane = node kernels, the slot kernel);
    // what it leaves goes to the per-pass kernels (StreamPlan::rp).
    // (the entry points have said so already, before staging anything: nothing wrong is ever decoded from here either)
    { const int refused = decode_gate(h, h->row_probs ? "per-row channel probabilities are" : nullptr, false); if (refused) return refused; }
    if (h->variant == Variant::Decimation) return decode_onchip_gd(h, synd, batch, decoding, llr, iters, conv);  // guided decimation: the lane = edge kernels or a refusal, never another family
    if (h->variant == Variant::Relay) return decode_relay(h, synd, batch, decoding, llr, iters, conv);
    if (h->msg_dtype == LDPC_HIP_MSG_F32) return decode_f32(h, synd, batch, decoding, llr, iters, conv);  // (never an FP64 kernel: what the mode cannot do is refused there)
    const bool rp = h->row_probs != nullptr;
    if (rp && h->schedule != 1) return fail(LDPC_HIP_ERR_UNSUPPORTED, "per-row channel probabilities: the serial schedules read the handle's priors only (parallel schedule required)");
    if (h->schedule == 0 || h->schedule == 2) return decode_serial(h, synd, batch, decoding, llr, iters, conv);
    {   // small code: the kernels that keep a syndrome's messages on chip (tu_onchip.hip), where one applies
        bool took = false;
        const int rc_onchip = decode_onchip(h, synd, batch, decoding, llr, iters, conv, &took);
        if (took || rc_onchip) return rc_onchip;
    }
    // streamed tiles: a tile runs until the slowest of its 64 syndromes is done.  Where most syndromes converge early
    // a short first pass + a second pass over the compacted rest does the same work in a fraction of the tile-iterations
    // (switch REPACK_MIN_TILES t > 0: t instead of the 512 tiles -- the tests cut batches of a few dozen tiles with it)
    const int64_t min_tiles = h->sw("REPACK_MIN_TILES") > 0 ? h->sw("REPACK_MIN_TILES") : 512;
    // (memory min-sum is not cut in two passes: the compaction would have to gather M too -- DESIGN.md section 7c)
    if (!rp && h->variant != Variant::Memory && h->repack_iters != 0 && h->max_iter >= 8 && tiles_total >= min_tiles && h->m > 0 && h->n > 0)
        return decode_stream_repacked(h, synd, batch, decoding, llr, iters, conv);
    return decode_streamed(h, synd, batch, decoding, llr, iters, conv, StreamPass());
}
