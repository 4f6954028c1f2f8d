// host_osd.h -- host side of OSD: list, kernel choice by size, status, second pass for syndromes outside the image
// Part of libldpc_hip.so: included by tu_osd.hip.
#pragma once

// H bit-packed by rows, `stride` 64-bit words per row (bit c of a row = its entry in column c)
static std::vector<uint64_t> pack_rows(const ldpc_hip_bp *h, size_t stride) {
    std::vector<uint64_t> mat((size_t)h->m * stride, 0);
    for (int i = 0; i < h->m; ++i)
        for (int e = h->h_row_ptr[(size_t)i]; e < h->h_row_ptr[(size_t)i + 1]; ++e) {
            const int c = h->h_col_idx[(size_t)e];
            mat[(size_t)i * stride + (size_t)(c >> 6)] |= 1ull << (c & 63);
        }
    return mat;
}
// k = n - rank(H) over GF(2): how many non-pivot columns an OSD elimination leaves (independent of the column order)
static int osd_k(ldpc_hip_bp *h) {
    if (h->osd_k_cached >= 0) return h->osd_k_cached;
    const int m = h->m, n = h->n, W = (n + 63) / 64;
    std::vector<uint64_t> mat = pack_rows(h, (size_t)W);
    int rank = 0;
    for (int c = 0; c < n && rank < m; ++c) {
        int p = -1;
        for (int i = rank; i < m; ++i)
            if ((mat[(size_t)i * W + (size_t)(c >> 6)] >> (c & 63)) & 1ull) { p = i; break; }
        if (p < 0) continue;
        for (int w = 0; w < W; ++w) std::swap(mat[(size_t)p * W + w], mat[(size_t)rank * W + w]);
        for (int i = 0; i < m; ++i)
            if (i != rank && ((mat[(size_t)i * W + (size_t)(c >> 6)] >> (c & 63)) & 1ull))
                for (int w = 0; w < W; ++w) mat[(size_t)i * W + w] ^= mat[(size_t)rank * W + w];
        ++rank;
    }
    h->osd_k_cached = n - rank;
    return h->osd_k_cached;
}

// a host table the OSD kernels read, uploaded once per handle
static int upload_once(DeviceBuf &buf, const void *data, size_t bytes) {
    int rc;
    if ((rc = buf.ensure(bytes))) return rc;
    HIPCHK(hipMemcpy(buf.p, data, bytes, hipMemcpyHostToDevice));
    return LDPC_HIP_OK;
}
// OsdArgs::ell: a row's entries as eight 16-bit column numbers, 0xffff behind them
static int ensure_osd_ell(ldpc_hip_bp *h) {
    if (h->osd_ell.p) return LDPC_HIP_OK;
    std::vector<uint16_t> ell((size_t)h->m * 8, (uint16_t)0xffff);
    for (int i = 0; i < h->m; ++i)
        for (int e = h->h_row_ptr[(size_t)i], k = 0; e < h->h_row_ptr[(size_t)i + 1]; ++e, ++k) ell[(size_t)i * 8 + (size_t)k] = (uint16_t)h->h_col_idx[(size_t)e];
    return upload_once(h->osd_ell, ell.data(), ell.size() * 2);
}

// Which kernel an OSD call reaches and how it is launched: worked out once per bposd_device call (plan_osd), used by both passes (launch_osd)
struct OsdPlan {
    const void *kernel;
    bool big;            // osd_big_kernel: its argument block is `big` with `o` filled in, else `a` alone
    OsdArgs a;           // what the matrix, the method and the order settle (LDS per wavefront among them); batch and the per-pass pointers are the caller's
    OsdBigArgs big_args;
    int waves;           // wavefronts per workgroup
    size_t lds;          // dynamic LDS of a workgroup, bytes
    int64_t grid;        // workgroups
    bool writes_status;  // the kernel says itself what became of a row (else osd_status_kernel afterwards)
};

static int plan_osd_big(ldpc_hip_bp *h, bool higher, bool host_rank, int64_t batch, OsdPlan &P) {
    const OsdArgs &a = P.a;
    OsdBigArgs &A = P.big_args;
    if (a.m > 32767 || a.n > 32767)
        return fail(LDPC_HIP_ERR_UNSUPPORTED, "OSD on the device: %d x %d is beyond the 16-bit row / column tables of the workgroup kernel", a.m, a.n);
    A.hwords = (a.n + 63) / 64;
    A.pow2 = 1;
    while (A.pow2 < a.n) A.pow2 <<= 1;
    A.max_rank = a.rank;
    A.kwords = !higher ? 0 : host_rank ? (a.n - a.rank + 63) / 64 : A.hwords;  // planes of T; rank unknown: room for every column
    if (higher && A.kwords < 1) A.kwords = 1;
    // blocked elimination (osd_block_eliminate): up to eight rows per thread in registers -> m <= 2048, and the combination table
    // of the block's pivot rows in LDS; LDPC_HIP_OSD_UNBLOCKED=1 keeps the one-pivot-per-step loop (A/B measurements)
    const bool blocked = a.m <= OSD_BLOCK_ROWS && !h->on("OSD_UNBLOCKED");
    auto room_end = [&](int nplanes) { return osd_big_lds_bytes(a.m, a.n, A.pow2, A.hwords, blocked, nplanes); };
    auto per_cu = [](size_t lds) {  // resident workgroups (+ the kernel's static LDS)
        const int pc = (int)((160u * 1024u) / (lds + 1024));
        return pc > 4 ? 4 : pc < 1 ? 1 : pc;
    };
    // the staged T planes, one buffer of 8 (m + 1) bytes per wavefront that weighs candidates: four, unless fewer let more
    // workgroups stay resident (tall matrices: at 1728 rows four buffers are 55 KiB and leave ONE workgroup per CU) -- weighing is
    // about a quarter of an OSD row, so halving its wavefronts costs ~ 25 %, a second resident workgroup gains ~ 70 %
    // -- IF there are more rows than resident workgroups; a handful of rows is about latency and wants all four.  How many rows the
    // previous OSD call on this handle listed is the guide (copied back asynchronously, never waited for; first call: an eighth of the batch).
    A.nplanes = 4;
    if (higher) {
        const unsigned seen = h->h_flag ? ((volatile unsigned *)h->h_flag)[8] : 0u;
        const double rows = seen ? (double)seen : (double)batch / 8.0 + 1.0;
        double best = 1e300;
        for (int nb = 4; nb >= 1; nb >>= 1) {
            const double cost = std::ceil(rows / (256.0 * per_cu(room_end(nb)))) * (1.0 + 0.25 * (4.0 / nb - 1.0));  // rounds of resident workgroups x time of a row
            if (cost < best - 1e-9) { best = cost; A.nplanes = nb; }
        }
        const int nb = h->sw("OSD_PLANES");  // (tests, measurements)
        if (nb == 1 || nb == 2 || nb == 4) A.nplanes = nb;
    }
    P.a.big_ord_off = (int32_t)osd_big_ord_off(a.m);
    A.extra_off = (int32_t)osd_big_room_off(a.m, A.pow2);
    A.pbuf_off = blocked ? (int32_t)osd_big_tbl_off((size_t)A.extra_off, a.m) : -1;
    size_t lds = room_end(higher ? A.nplanes : 0);
    if (lds > 150u * 1024u)
        return fail(LDPC_HIP_ERR_UNSUPPORTED, "OSD on the device: the column order%s of a %d x %d matrix need%s %zu bytes of LDS, 150 KiB available",
                    higher ? " and the candidate tables" : "", a.m, a.n, higher ? "" : "s", lds);
    lds = (lds + 15) & ~(size_t)15;
    const size_t mat_bytes = (size_t)A.hwords * a.m * 8;
    const bool mat_lds = !h->osd_big && lds + mat_bytes <= 150u * 1024u;
    if (mat_lds) { A.mat_off = (int32_t)lds; lds += mat_bytes; }
    A.slot_stride = (int64_t)((mat_lds ? 0 : A.hwords) + A.kwords) * a.m;
    if (A.slot_stride < 1) A.slot_stride = 1;
    int64_t slots = 256 * (int64_t)per_cu(lds);
    if (slots > batch) slots = batch;
    const int64_t cap = (int64_t)(4ull << 30) / (A.slot_stride * 8);  // at most 4 GiB of working copies
    if (slots > cap) slots = cap > 0 ? cap : 1;
    int rc;
    if ((rc = h->osd_scratch.ensure((size_t)slots * (size_t)A.slot_stride * 8))) return rc;
    A.scratch = (uint64_t *)h->osd_scratch.p;
    void (*bk)(const OsdBigArgs) = higher ? (mat_lds ? osd_big_kernel<true, true> : osd_big_kernel<true, false>)
                                          : (mat_lds ? osd_big_kernel<false, true> : osd_big_kernel<false, false>);
    P.big = true; P.kernel = (const void *)bk;
    P.waves = 4; P.lds = lds; P.grid = slots;
    return LDPC_HIP_OK;
}

static int plan_osd(ldpc_hip_bp *h, int osd_method, int osd_order, int64_t batch, OsdPlan *plan) {
    OsdPlan &P = *plan;
    P = {};
    OsdArgs &a = P.a;
    const bool higher = osd_method >= 2 && osd_order > 0;  // osd_order == 0 takes the OSD-0 branch whatever the method (osd.hpp:114)
    a.m = h->m; a.n = h->n; a.words = (h->n + 1 + 63) / 64;
    a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx;
    a.method = osd_method; a.order = osd_order; a.wt = h->d_osd_wt;
    if (osd_method == 3 && osd_order > 0) {
        // OSD_CS pairs (i, j), i < j < osd_order, are listed i-major and only those with j < k = n - rank exist in the reference's
        // candidate strings (osd.hpp:91-99; beyond: a write past the string).  Their order in the list -- which is all an index is
        // used for: the earliest of equally light candidates wins -- does not depend on osd_order once it is >= k, so a larger
        // order is the same sweep as order k (and the kernels need not walk millions of pair numbers that name nothing).
        const int k_bound = (double)a.m * a.m * a.words < 4e9 ? osd_k(h) : a.n;
        if (a.order > k_bound) a.order = k_bound > 0 ? k_bound : 1;
    }
    int rc;
    // small matrices: the elimination runs in registers (<R, W>: m <= 64 R, n + 1 <= 64 W), LDS only holds the column order (and, higher
    // order, the column records).  (BB [[144,12,12]]: 72 x 145 bits -> <2, 3> -- a fourth word would be a quarter more sort and XOR work)
    const int rung = !h->osd_reg || h->osd_big ? -1 : a.m <= 64 && a.words <= 2 ? 0 : a.m <= 128 && a.words <= 3 ? 1 : a.m <= 128 && a.words <= 4 ? 2
                   : a.m <= 256 && a.words <= 8 ? 3 : -1;
    size_t per_wave;
    if (rung >= 0 && !higher) {
        static void (*const reg0[4])(const OsdArgs) = {osd0_reg_kernel<1, 2>, osd0_reg_kernel<2, 3>, osd0_reg_kernel<2, 4>, osd0_reg_kernel<4, 8>};
        P.kernel = (const void *)reg0[rung];
        per_wave = ((size_t)a.n * 4 + 15) & ~(size_t)15;  // order [n] i32
        // ... and with the columns permuted into their sorted order where the matrix allows (osd0_flat_kernel: m <= 128, n <= 256, rows of up to
        // eight entries): half the instructions per pivot, and a small batch's OSD stage lasts as long as its slowest row
        if (a.m <= 128 && a.n <= 256 && h->max_row_deg <= 8 && !h->on("OSD_NO_FLAT")) {
            static void (*const flat[2][4])(const OsdArgs) = {{osd0_flat_kernel<1, 2>, osd0_flat_kernel<1, 3>, osd0_flat_kernel<1, 5>, osd0_flat_kernel<1, 8>},
                                                              {osd0_flat_kernel<2, 2>, osd0_flat_kernel<2, 3>, osd0_flat_kernel<2, 5>, osd0_flat_kernel<2, 8>}};
            static const int flat_ds[4] = {2, 3, 5, 8};
            const int need = (a.n + 31) / 32, flat_r = a.m <= 64 ? 1 : 2;
            int q = 0;
            while (flat_ds[q] < need) ++q;
            P.kernel = (const void *)flat[flat_r - 1][q];
            per_wave = osd_flat_lds_bytes(a.n, flat_r, flat_ds[q]);
            if ((rc = ensure_osd_ell(h))) return rc;
            a.ell = (const uint16_t *)h->osd_ell.p;
        }
    } else if (rung >= 0) {
        static void (*const regw[4])(const OsdArgs) = {osdw_reg_kernel<1, 2>, osdw_reg_kernel<2, 3>, osdw_reg_kernel<2, 4>, osdw_reg_kernel<4, 8>};
        P.kernel = (const void *)regw[rung];
        a.kwords = (osd_k(h) + 63) / 64;
        if (a.kwords < 1) a.kwords = 1;
        per_wave = osdw_reg_lds(a.n, a.kwords).total;
    } else {
        P.kernel = higher ? (const void *)osdw_kernel : (const void *)osd0_kernel;
        per_wave = osd_lds_layout(a.m, a.n, a.words, higher).total;
    }
    P.writes_status = rung >= 0 && !higher;
    // one workgroup per syndrome (osd_big_kernel) once the one-wavefront kernels would leave fewer than four wavefronts on a CU;
    // mode 0 keeps the one-wavefront kernels while they fit at all
    const bool big = rung < 0 && (per_wave > 150u * 1024u || h->osd_big || (h->osd_reg && per_wave > 40u * 1024u));
    if (rung >= 0 || big) {
        // rank H bounds the pivots; working it out is a dense elimination on the host, worth it only for moderate sizes
        const bool host_rank = rung >= 0 || (double)a.m * a.m * a.words < 4e9;
        a.rank = host_rank ? a.n - osd_k(h) : (a.m < a.n ? a.m : a.n);
        if (!h->osd_packed.p && (rc = upload_once(h->osd_packed, pack_rows(h, (size_t)a.words).data(), (size_t)a.m * a.words * 8))) return rc;  // (bit n, the syndrome's place, clear)
        a.packed = (const uint64_t *)h->osd_packed.p;
        if (big) return plan_osd_big(h, higher, host_rank, batch, P);
    }
    // wavefronts per workgroup: whichever of 1..4 lets most wavefronts reside on a CU (a workgroup's LDS is one
    // allocation, so large per-wavefront tables pack better in small workgroups); ties go to the larger workgroup
    int resident_best = 0;
    P.waves = 1;
    for (int w = 1; w <= 4; ++w) {
        if ((size_t)w * per_wave > 150u * 1024u) break;
        int resident = (int)((160u * 1024u) / ((size_t)w * per_wave)) * w;
        if (resident > 32) resident = 32;
        if (resident >= resident_best) { resident_best = resident; P.waves = w; }
    }
    a.lds_per_wave = (int32_t)per_wave;
    P.lds = per_wave * (size_t)P.waves;
    // persistent wavefronts (as many as LDS lets reside) pull rows from the list
    int groups_per_cu = (int)((160u * 1024u) / P.lds);
    if (groups_per_cu * P.waves > 32) groups_per_cu = 32 / P.waves;
    if (groups_per_cu < 1) groups_per_cu = 1;
    P.grid = 256 * (int64_t)groups_per_cu;
    if (P.grid > (batch + P.waves - 1) / P.waves) P.grid = (batch + P.waves - 1) / P.waves;
    return LDPC_HIP_OK;
}

// the planned OSD kernel over the rows of a.list
static int launch_osd(ldpc_hip_bp *h, const OsdPlan &P, const OsdArgs &a) {
    OsdBigArgs A = P.big_args;
    A.o = a;
    void *params[] = {P.big ? (void *)&A : (void *)&a};
    HIPCHK(LDPC_LAUNCH_PTR(P.kernel, dim3((unsigned)P.grid), dim3((unsigned)(P.waves * 64)), params, P.lds, h->stream));
    return LDPC_HIP_OK;
}

// Rows whose syndrome lies outside the image of H (status 2; only a rank-deficient H has any): the reference's answer depends on
// which rows its linked-list elimination made pivot rows.  One workgroup per such row re-enacts that choice and writes the syndrome
// that keeps exactly those rows (osd_exact_kernel.h); the same OSD kernel then runs once more over these rows.  No host round trip:
// both launches size themselves from device-side counters and cost a few microseconds when there is nothing to do.
static int osd_second_pass(ldpc_hip_bp *h, const OsdPlan &P, const OsdArgs &a) {
    if ((double)a.m * a.m * a.words >= 4e9 /* rank unknown */ || a.n - osd_k(h) >= a.m || a.m > 8192) return LDPC_HIP_OK;
    // Footprint (documented in ldpc_hip.h): at most 64 workgroups' working copies, capped at 256 MiB, plus one corrected syndrome and
    // one list entry per row of the batch.  If the device cannot spare that, the second pass is skipped -- the first-pass solutions
    // stand and the affected rows keep status 2 -- rather than failing a decode whose outputs are already complete.
    const size_t B = (size_t)a.batch, slot_words = osd_exact_slot_words(a.m, a.n);
    int64_t slots = 64;
    if (slots > a.batch) slots = a.batch;
    const int64_t cap = (int64_t)((256ull << 20) / (slot_words * 8));
    if (cap < 1) return LDPC_HIP_OK;
    if (slots > cap) slots = cap;
    if (h->osd_fix_synd.ensure(B * (size_t)a.m) || h->osd_fix_list.ensure(B * sizeof(int32_t)) ||
        h->osd_fix_scratch.ensure((size_t)slots * slot_words * 8)) {
        (void)hipGetLastError();  // out of memory: not an error of this decode
        g_last_error.clear();
        return LDPC_HIP_OK;
    }
    OsdExactArgs X = {};
    X.o = a;
    X.status = (const uint8_t *)h->osd_status.p;
    X.corrected = (uint8_t *)h->osd_fix_synd.p;
    X.list2 = (int32_t *)h->osd_fix_list.p;
    X.counters2 = osd_counter_ptr(h) + 8;
    X.scratch = (uint64_t *)h->osd_fix_scratch.p;
    X.slot_words = (int64_t)slot_words;
    X.hw = (a.n + 63) / 64;
    const size_t xl = osd_exact_lds_bytes(a.m);
    if (xl > 48u * 1024u) HIPCHK(hipFuncSetAttribute((const void *)osd_exact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)xl));
    LDPC_LAUNCH(osd_exact_kernel, dim3((unsigned)slots), dim3(256), (unsigned)xl, h->stream, X);
    HIPCHK(hipGetLastError());
    OsdArgs a2 = a;
    a2.synd = X.corrected;
    a2.list = X.list2;
    a2.counters = X.counters2;
    a2.status = nullptr;  // (these rows keep their 2)
    return launch_osd(h, P, a2);
}

// BP, then OSD on the rows BP left unconverged; device pointers, on h->stream
int bposd_device(ldpc_hip_bp *h, int osd_method, int osd_order, const uint8_t *synd, int64_t batch, uint8_t *decoding,
                        double *llr, int32_t *iters, uint8_t *conv) {
    if (osd_method == 0)  // OSD_OFF: BpOsdDecoder still calls OsdDecoder::decode, which then has no LU object -- refuse instead
        return fail(LDPC_HIP_ERR_INVALID, "osd_method is OSD_OFF");
    const size_t B = (size_t)batch, n = (size_t)h->n;
    int rc;
    if (!llr) { if ((rc = h->osd_llr.ensure(B * n * 8 ? B * n * 8 : 1))) return rc; llr = (double *)h->osd_llr.p; }
    if (!conv) { if ((rc = h->osd_conv.ensure(B ? B : 1))) return rc; conv = (uint8_t *)h->osd_conv.p; }
    h->osd_status_rows = 0;
    // The counters of the OSD passes -- {listed, next} of the first at [0..1], of the second (rows outside the image) at [8..9] -- sit behind the
    // BP kernels' work pools, so that ONE fill serves both, and an on-chip BP kernel lists the rows it leaves unconverged and clears the
    // status array itself (osd_hook; otherwise osd_collect_kernel does both below): every launch costs 4 - 5 us whatever it does, and at
    // BASELINE config 5's 8 192 rows the eight small ones around BP and OSD-0 were a tenth of the step.
    if ((rc = h->counter.ensure(counter_bytes()))) return rc;
    if ((rc = h->osd_list.ensure((B ? B : 1) * sizeof(int32_t)))) return rc;
    if ((rc = h->osd_status.ensure(B ? B : 1))) return rc;
    unsigned *const osd_ctr = osd_counter_ptr(h);
    // (row priors: the kernels that take them have no hand-over of their own -- the rows are collected afterwards, as under OSD_COLLECT_AFTER;
    //  OSD-0 itself orders the columns by BP's posteriors, which are per row already: it needs no prior)
    h->osd_hook = {(int32_t *)h->osd_list.p, osd_ctr, (uint8_t *)h->osd_status.p, !h->on("OSD_COLLECT_AFTER") && !h->row_probs, false};
    rc = decode_device(h, synd, batch, decoding, llr, iters, conv);
    h->osd_hook.armed = false;
    if (rc) return rc;
    if (h->m == 0 || h->n == 0) return LDPC_HIP_OK;
    OsdPlan P;
    if ((rc = plan_osd(h, osd_method, osd_order, batch, &P))) return rc;
    if (P.lds > 48u * 1024u) HIPCHK(hipFuncSetAttribute(P.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
    OsdArgs a = P.a;
    a.batch = batch; a.synd = synd; a.llr = llr; a.conv = conv; a.decoding = decoding;
    a.list = (const int32_t *)h->osd_list.p;
    a.counters = osd_ctr;
    a.status = P.writes_status ? (uint8_t *)h->osd_status.p : nullptr;
    if (!h->osd_hook.done) {  // list the unconverged rows
        HIPCHK(hipMemsetAsync(osd_ctr, 0, OSD_COUNTER_BYTES, h->stream));
        LDPC_LAUNCH(osd_collect_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, conv, batch,
                           (int32_t *)h->osd_list.p, osd_ctr, (uint8_t *)h->osd_status.p);
    }
    h->osd_status_rows = batch;
    if ((rc = launch_osd(h, P, a))) return rc;
    if (P.big && h->h_flag) HIPCHK(hipMemcpyAsync(&h->h_flag[8], a.counters, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));  // rows listed: the next call's guide
    if (!P.writes_status) {  // did every OSD output solve its syndrome?  (the array was cleared on the way -- by the BP kernel or by osd_collect_kernel)
        const int64_t blocks = batch < 4096 ? batch : 4096;
        LDPC_LAUNCH(osd_status_kernel, dim3((unsigned)(blocks ? blocks : 1)), dim3(256), 0, h->stream, a, (uint8_t *)h->osd_status.p);
        HIPCHK(hipGetLastError());
    }
    return osd_second_pass(h, P, a);
}
