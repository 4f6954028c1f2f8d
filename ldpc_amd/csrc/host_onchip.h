// host_onchip.h -- host side of the on-chip kernels: plans (LDS / occupancy), tables and launches of bp_small / bp_wave / bp_wave_ps / bp_edge / bp_wave_relay / bp_wave_gd / bp_wave_f32 / bp_wave_rp
// Part of libldpc_hip.so: included by bp_hip.hip (one translation unit), in the order given there.
#pragma once


// what a decode is given (decode_onchip and its kin hand it on): device pointers, on h->stream
struct DecodeIo {
    const uint8_t *synd;
    int64_t batch;
    uint8_t *decoding;
    double *llr;
    int32_t *iters;
    uint8_t *conv;
};

// What every on-chip route asks before any plan: a code, small enough for the plans' tables, and a batch whose syndrome indices fit the work
// pools' 32 bits.  Each caller's own small-mode rule stands beside its call.
static bool onchip_bound(const ldpc_hip_bp *h, int64_t batch) {
    return h->m > 0 && h->n > 0 && h->nnz > 0 && (int64_t)h->nnz * 16 < (1 << 22) && batch < (1ll << 30);
}

// LDS bytes of the on-chip kernel for `slots` resident syndromes; 0 if the code is too large for it
static size_t small_lds_bytes(const ldpc_hip_bp *h, int slots, bool rp = false) {
    size_t fixed = 256 * 8 + (size_t)h->n * 8 + ((size_t)h->m + 1 + h->nnz + h->n + 1 + h->nnz) * 4;
    fixed = (fixed + 15) & ~(size_t)15;
    return fixed + small_slot_bytes(h->m, h->n, h->nnz, rp) * (size_t)slots;
}

// On-chip variant (bp_small_kernel): chosen automatically when four resident syndromes per workgroup still
// leave room for four workgroups per CU.  Device pointers, on h->stream.
static int decode_small(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr,
                        int32_t *iters, uint8_t *conv, int slots) {
    int rc;
    if ((rc = h->counter.ensure(8))) return rc;
    HIPCHK(hipMemsetAsync(h->counter.p, 0, 8, h->stream));
    SmallArgs a = {};
    a.m = h->m; a.n = h->n; a.nnz = h->nnz; a.max_iter = h->max_iter; a.slots = slots;
    a.ms_scaling_factor = h->ms_scaling_factor;
    a.batch = batch;
    a.row_ptr = h->d_row_ptr; a.col_idx = h->d_col_idx; a.col_ptr = h->d_col_ptr; a.csc_edge = h->d_csc_edge;
    a.llr0 = h->d_llr0;
    a.synd = synd; a.decoding = decoding; a.llr = llr; a.iters = iters; a.conv = conv;
    a.next = (unsigned long long *)h->counter.p;
    const bool rp = h->row_probs != nullptr;
    if (rp) {  // every syndrome's own priors, whole batch (a slot reads the lane of the syndrome it holds)
        const int64_t tiles = (batch + LDPC_WAVE - 1) / LDPC_WAVE;
        if ((rc = h->rowp_llr.ensure(sizeof(double) * (size_t)h->n * LDPC_WAVE * (size_t)tiles))) return rc;
        const dim3 gp((unsigned)((h->n + LDPC_WAVE - 1) / LDPC_WAVE), (unsigned)(tiles < 32768 ? tiles : 32768));
        LDPC_LAUNCH(row_priors_kernel, gp, dim3(256), 0, h->stream, h->row_probs, batch, h->n, (const double *)h->d_llr0, (double *)h->rowp_llr.p);
        HIPCHK(hipGetLastError());
        a.llr0_t = (const double *)h->rowp_llr.p;
    }
    void (*kern)(const SmallArgs) = rp ? with_method_math(h, [](auto M, auto F) { return &bp_small_kernel<M, F, true>; })
                                       : with_method_math(h, [](auto M, auto F) { return &bp_small_kernel<M, F>; });
    const size_t dyn = small_lds_bytes(h, slots, rp);
    if (dyn > 48u * 1024u)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    // persistent workgroups: enough to fill the chip, never more than there are syndromes to hand out
    int64_t groups = (batch + slots - 1) / slots;
    const int64_t resident = 256 * (int64_t)((150u * 1024u) / dyn > 8 ? 8 : (150u * 1024u) / dyn);
    if (groups > resident) groups = resident;
    h->accumulated_ms = 0.f;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    LDPC_LAUNCH(kern, dim3((unsigned)groups), dim3(256), (unsigned)dyn, h->stream, a);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// bp_wave_kernel: template bounds, launch shape and LDS split; waves == 0: not applicable (degrees, table range, LDS)
// the priors as bp_wave_kernel's LDS copy would hold them: llr0, 1.0 for the padding columns, DBL_MAX at np (a row's phantom entries)
__global__ void wave_prior_pad_kernel(const double *llr0, int n, int np, double *out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < np + 2) out[q] = q < n ? llr0[q] : q == np ? DBL_MAX : 1.0;
}

struct WavePlan {
    int dr = 0, dc = 0, waves = 0, groups_per_cu = 0, mp = 0, np = 0;
    size_t shared = 0, per_wave = 0;
    bool llr_direct = false;
    bool prior_global = false;  // min-sum: the priors are read from a padded device array instead of an LDS copy (WaveArgs.prior_g)
    bool team = false;  // the workgroup's wavefronts share ONE syndrome (bp_wave_kernel<..., TEAM>): `waves` = wavefronts of a team
    void (*kern)(const WaveArgs) = nullptr, (*kern_team)(const WaveArgs) = nullptr;
};

// The rungs (rows <=, columns <=) of the lane = node and lane = entry kernels, ascending: a code takes the first that holds it.  The first four are
// bp_wave_ps_kernel's too (pick_wave_ps, which goes on with rungs of its own); all six are bp_wave_kernel's, bp_wave_relay_kernel's, bp_wave_gd_kernel's, bp_wave_f32_kernel's and bp_wave_rp_kernel's.
#define LDPC_WAVE_LADDER4(X) X(4, 2) X(4, 4) X(6, 3) X(8, 4)
#define LDPC_WAVE_LADDER(X) LDPC_WAVE_LADDER4(X) X(8, 8) X(16, 8)

template <int METHOD, int MATH>
static void pick_wave(int max_row, int max_col, WavePlan &p) {
    // rows of up to 16 entries (hamming(5) as a full parity-check matrix): min-sum only -- product-sum takes the lane = entry kernel there
    // (bp_wave_ps_kernel<., 16 | 32, 8>), and its lane = node form would need more registers than a 16-wavefront workgroup has
#define LDPC_RUNG(R, C) \
    if constexpr (R <= 8 || METHOD == LDPC_HIP_MINIMUM_SUM) \
        if (!p.kern && max_row <= R && max_col <= C) { p.dr = R; p.dc = C; p.kern = bp_wave_kernel<METHOD, MATH, R, C, false>; p.kern_team = bp_wave_kernel<METHOD, MATH, R, C, true>; }
    LDPC_WAVE_LADDER(LDPC_RUNG)
#undef LDPC_RUNG
}

// ---- the rules plan_wave and plan_wave_lds share, each stated once ----
// rows and columns padded to whole wavefronts; false: a table entry would not fit (positions and column numbers are 16 bits)
static bool wave_pad(const ldpc_hip_bp *h, WavePlan &p) {
    p.mp = (h->m + 63) / 64 * 64;
    p.np = (h->n + 63) / 64 * 64;
    return !((size_t)p.dr * p.mp + 2 >= 65536 || p.np + 1 >= 65536);
}
// a few heavy rows would pad every row (a plan that was not forced refuses)
static bool wave_padding_dominates(const ldpc_hip_bp *h, const WavePlan &p) { return (size_t)p.dr * p.mp > 2 * (size_t)h->nnz + 1024; }
// Do the workgroup's wavefronts share ONE syndrome?  w: the wavefronts LDS has room for, one syndrome each; u: the kernel's nodes per lane in flight.
// small_mode 5 forces, 4 forbids it; the reasons and the measurements stand in plan_wave.
static bool wave_team_rule(const ldpc_hip_bp *h, const WavePlan &p, size_t w, int u, int64_t batch) {
    return h->small_mode == 5 || (h->small_mode != 4 && (w < 6 || 2 * p.np > 3 * 64 * u || batch <= 256 * (int64_t)w));
}
// a team: as many wavefronts as its bit pass has rounds of 64 u columns for, two at least, `cap` at most
static int wave_team_width(const WavePlan &p, int u, int cap) {
    const int tw = (p.np + 64 * u - 1) / (64 * u);
    return tw < 2 ? 2 : tw > cap ? cap : tw;
}
// teams per compute unit, sixteen wavefronts in all
// (bp_wave_kernel's ~100 VGPRs allow 16 wavefronts per CU: two teams of eight beat one of thirteen -- 768 x 1600: 4.0 vs 4.8 ms)
static void wave_team_groups(WavePlan &p, size_t lds) {
    p.groups_per_cu = (int)(lds / (p.shared + p.per_wave));
    if (p.groups_per_cu >= 2 && p.waves > 8) p.waves = 8;
    if (p.groups_per_cu * p.waves > 16) p.groups_per_cu = 16 / p.waves;
    if (p.groups_per_cu < 1) p.groups_per_cu = 1;
}
// workgroups of p.waves wavefronts, one syndrome each, per compute unit: `cap` wavefronts in all
static void wave_solo_groups(WavePlan &p, size_t lds, int cap) {
    p.groups_per_cu = (int)(lds / (p.shared + (size_t)p.waves * p.per_wave));
    if (p.groups_per_cu * p.waves > cap) p.groups_per_cu = cap / p.waves;
    if (p.groups_per_cu < 1) p.groups_per_cu = 1;
}

// The LDS copy of the log-ratios is a convenience (the store of every iteration stays on chip); where it costs a resident wavefront and few are
// resident, every bit pass stores them straight to HBM instead.  copy / lean: a syndrome's private bytes with and without the copy.
static bool wave_llr_direct_rule(size_t lds, size_t shared, size_t copy, size_t lean) {
    const size_t w_copy = shared + copy > lds ? 0 : (lds - shared) / copy;
    const size_t w_lean = shared + lean > lds ? 0 : (lds - shared) / lean;
    return w_copy < 4 && w_lean > w_copy;
}

static WavePlan plan_wave(const ldpc_hip_bp *h, bool forced, bool want_llr, int64_t batch) {
    WavePlan p;
    if (h->m <= 0 || h->n <= 0 || h->nnz <= 0 || h->max_row_deg > 16 || h->max_col_deg > 8) return p;
    with_method_math(h, [&](auto M, auto F) { pick_wave<M, F>(h->max_row_deg, h->max_col_deg, p); });
    if (!p.kern) return p;
    if (!wave_pad(h, p) || (!forced && wave_padding_dominates(h, p))) return p;
    p.shared = wave_lds_shared(p.mp, p.np, p.dr, p.dc, h->bp_method == LDPC_HIP_PRODUCT_SUM);
    p.per_wave = wave_lds_private(p.mp, p.np, p.dr, want_llr);
    // one workgroup per compute unit with as many wavefronts as LDS (160 KiB) and the 16-wave workgroup limit allow;
    // small codes fit several such workgroups
    const size_t lds = 160u * 1024u - 64u;  // (the kernels' few bytes of static LDS come on top of the dynamic part)
    if (want_llr) {
        const size_t lean = wave_lds_private(p.mp, p.np, p.dr, false);
        if (wave_llr_direct_rule(lds, p.shared, p.per_wave, lean)) { p.per_wave = lean; p.llr_direct = true; }
    }
    if (p.shared + p.per_wave > lds) return p;
    size_t w = (lds - p.shared) / p.per_wave;
    if (w > 16) w = 16;
    // Few resident wavefronts hide little latency, but a wavefront stops when ITS syndrome has converged while a streamed
    // tile runs until its slowest of 64 has.  Measured on 432..864-row window matrices (tools/bench_window.py): min-sum
    // with 3 / 2 / 1 wavefronts per CU is 12x / 7x / 1.5x faster than streaming when most syndromes converge early and
    // 2.2x faster at 3 when most do not; product-sum 3x / 2.4x / 0.7x and about level.
    // Where LDS leaves room for only a few syndromes per CU, one wavefront each leaves the CU idle: the wavefronts of a workgroup
    // then share ONE syndrome (TEAM), as many as its bit pass has rounds of 64 U columns for (small_mode 5 forces, 4 forbids it);
    // and a code whose bit pass takes one wavefront several rounds is quicker that way whatever the room.
    // Measured (round 2, min-sum / product-sum, large batches): 768 x 1600 15.5 -> 4.9 ms / 50 -> 16 ms, 1200 x 2400 21 -> 3.5 ms,
    // surface d = 41 / 31 / 21 25 -> 11 / 24 -> 12.6 / 11.0 -> 10.0 ms, 300 x 600 1.03 -> 0.79 ms; d = 13, 17 (the bit pass of one
    // wavefront is a single round of 64 U columns already) 7 % slower -- hence the second condition.
    const bool ms = h->bp_method == LDPC_HIP_MINIMUM_SUM;
    const int u = ms ? wave_ms_nodes_per_lane(p.dr, 1) : (p.dr <= 6 ? 2 : 1);  // the kernel's nodes per lane in flight (min-sum: the row part)
    // A batch of no more than one syndrome per wavefront slot is about latency: a team (two wavefronts at least) then too --
    // surface d = 9 .. 17, BB144 at 512 / 4 096 syndromes: 1.25 - 1.6x / 1.0 - 1.3x faster, at 65 536 up to 16 % slower.
    if (wave_team_rule(h, p, w, u, batch)) {
        p.team = true;
        p.waves = wave_team_width(p, u, 16);
        p.kern = p.kern_team;
        if (ms) {  // the LDS copy of the priors, 8 (np + 2) bytes: worth reading them from memory where that fits another workgroup
            const size_t lean_shared = wave_lds_shared(p.mp, p.np, p.dr, p.dc, false, false);
            if (lds / (lean_shared + p.per_wave) > lds / (p.shared + p.per_wave)) { p.shared = lean_shared; p.prior_global = true; }
        }
        wave_team_groups(p, lds);
        return p;
    }
    if (!forced && w < (ms ? 2 : 3)) return p;
    p.waves = (int)w;
    wave_solo_groups(p, lds, 32);  // 32 wavefronts per compute unit
    return p;
}

// structure-of-arrays position tables of bp_wave_kernel for the bounds (dr, dc): see bp_wave_kernel.h
static int ensure_wave_tables(ldpc_hip_bp *h, const WavePlan &p) {
    if (h->wave_dr == p.dr && h->wave_dc == p.dc) return LDPC_HIP_OK;
    const int m = h->m, n = h->n, mp = p.mp, np = p.np;
    const size_t rm = (size_t)p.dr * mp, cn = (size_t)p.dc * np;
    std::vector<uint8_t> rdeg((size_t)mp, 0), cdeg((size_t)np, 0);
    std::vector<uint16_t> wcol(rm, (uint16_t)np), wapos(cn, (uint16_t)(rm + 1));  // phantom defaults
    std::vector<int32_t> seen((size_t)n, 0);  // entries of column j met so far = rank of the next one inside the column
    for (int i = 0; i < m; ++i) {
        const int lo = h->h_row_ptr[(size_t)i];
        rdeg[(size_t)i] = (uint8_t)(h->h_row_ptr[(size_t)i + 1] - lo);
        for (int e = lo; e < h->h_row_ptr[(size_t)i + 1]; ++e) {
            const int k = e - lo, j = h->h_col_idx[(size_t)e], kc = seen[(size_t)j]++;  // rows ascend: kc is the CSC order
            wcol[(size_t)k * mp + i] = (uint16_t)j;
            wapos[(size_t)kc * np + j] = (uint16_t)((size_t)k * mp + i);
        }
    }
    for (int j = 0; j < n; ++j) cdeg[(size_t)j] = (uint8_t)seen[(size_t)j];
    int rc;
    if ((rc = h->w_rdeg.ensure(rdeg.size())) || (rc = h->w_cdeg.ensure(cdeg.size())) || (rc = h->w_col.ensure(rm * 2)) ||
        (rc = h->w_apos.ensure(cn * 2))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));  // a previous launch may still read the old tables
    HIPCHK(hipMemcpy(h->w_rdeg.p, rdeg.data(), rdeg.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->w_cdeg.p, cdeg.data(), cdeg.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->w_col.p, wcol.data(), rm * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->w_apos.p, wapos.data(), cn * 2, hipMemcpyHostToDevice));
    h->wave_dr = p.dr;
    h->wave_dc = p.dc;
    return LDPC_HIP_OK;
}

// bp_wave_ps_kernel (product-sum, lane = entry): bounds, launch shape, LDS split; waves == 0: not applicable
struct WavePsPlan {
    int dr = 0, dc = 0, waves = 0, groups_per_cu = 0, np = 0;
    size_t shared = 0, per_wave = 0;
    bool team = false;  // a workgroup per syndrome (bp_wave_ps_kernel<..., TEAM>): `waves` = wavefronts of a team
    void (*kern)(const WavePsArgs) = nullptr, (*kern_team)(const WavePsArgs) = nullptr;
};

template <int MATH>
static void pick_wave_ps(int max_row, int max_col, WavePsPlan &p) {
#define LDPC_RUNG(R, C) \
    if (!p.kern && max_row <= R && max_col <= C) { p.dr = R; p.dc = C; p.kern = bp_wave_ps_kernel<MATH, R, C, false>; p.kern_team = bp_wave_ps_kernel<MATH, R, C, true>; }
    LDPC_WAVE_LADDER4(LDPC_RUNG)
    // heavier rows (classical codes given as full parity-check matrices: hamming(5) has rows of 16, hamming(6) of 32): until round 4 these
    // fell to the workgroup ("slot") kernel, ~11 us of barriers per iteration -- a single decode() of hamming(5) took 230 us
    LDPC_RUNG(16, 8)
    LDPC_RUNG(32, 8)
#undef LDPC_RUNG
}

static WavePsPlan plan_wave_ps(const ldpc_hip_bp *h, bool forced, bool want_llr, int64_t batch) {
    WavePsPlan p;
    if (h->bp_method != LDPC_HIP_PRODUCT_SUM || h->m <= 0 || h->n <= 0 || h->nnz <= 0 || h->max_row_deg > 32 || h->max_col_deg > 8) return p;
    const bool heavy = h->max_row_deg > 8 || h->max_col_deg > 4;  // the (16, 8) / (32, 8) variants
    with_method_math(h, [&](auto M, auto F) {  // (product-sum only: see above)
        if constexpr (M == LDPC_HIP_PRODUCT_SUM) pick_wave_ps<F>(h->max_row_deg, h->max_col_deg, p);
    });
    p.np = (h->n + 63) / 64 * 64;
    const size_t rm = (size_t)p.dr * h->m;
    if (rm + 2 >= 65536 || (size_t)p.np + 1 >= 65536) return p;
    // padding would dominate (a heavy code's phantom column entries only cost unrolled LDS reads of the +0.0 slot: judged by its rows alone)
    if (!forced && (rm > 2 * (size_t)h->nnz || (!heavy && (size_t)p.dc * h->n > 2 * (size_t)h->nnz))) return p;
    p.shared = wave_ps_lds_shared(h->m, p.np, p.dr, p.dc);
    p.per_wave = wave_ps_lds_private(h->m, p.np, p.dr, want_llr);
    const size_t lds = 160u * 1024u - 64u;  // (the kernels' few bytes of static LDS come on top of the dynamic part)
    if (p.shared + p.per_wave > lds) return p;
    size_t w = (lds - p.shared) / p.per_wave;
    if (w > 16) w = 16;
    if (!forced && w < 8) return p;
    if (p.dr > 16 && w > 4) w = 4;  // (the kernel's launch bound: bp_wave_ps_kernel<., 32, .>)
    // A batch so small that every wavefront decodes only a few syndromes takes as long as its slowest syndrome: then the
    // workgroup's wavefronts share one (TEAM), one round of 64 entries each per pass.  LDPC_HIP_PS_TEAM=0 / 1 overrides (measurements).
    bool team = batch <= 256 * (int64_t)w * 8;  // (BB144, w = 16: 0.96 -> 0.57 ms at 8 192 syndromes, 1.52 -> 1.37 ms at 32 768, 4.2 -> 4.5 ms at 131 072)
    if (h->sw("PS_TEAM") >= 0) team = h->sw("PS_TEAM") != 0;
    if (team) {
        const size_t rounds = ((size_t)p.dr * h->m + 63) / 64;
        int tw = (int)(rounds < 2 ? 2 : rounds > 8 ? 8 : rounds);
        if (h->sw("PS_TEAM_WAVES") >= 1 && h->sw("PS_TEAM_WAVES") <= 16) tw = h->sw("PS_TEAM_WAVES");  // (measurements)
        if (p.dr > 16 && tw > 4) tw = 4;
        p.team = true;
        p.waves = tw;
        p.kern = p.kern_team;
        p.groups_per_cu = (int)(lds / (p.shared + p.per_wave));
        if (p.groups_per_cu * p.waves > 28) p.groups_per_cu = 28 / p.waves;  // (this kernel's 65 VGPRs allow 7 wavefronts per SIMD)
        if (p.groups_per_cu < 1) p.groups_per_cu = 1;
        return p;
    }
    p.waves = (int)w;
    p.groups_per_cu = (int)(lds / (p.shared + (size_t)p.waves * p.per_wave));
    if (p.groups_per_cu * p.waves > 32) p.groups_per_cu = 32 / p.waves;
    if (p.groups_per_cu < 1) p.groups_per_cu = 1;
    return p;
}

static int ensure_wave_ps_tables(ldpc_hip_bp *h, const WavePsPlan &p) {
    if (h->wave_ps_dr == p.dr && h->wave_ps_dc == p.dc) return LDPC_HIP_OK;
    const int m = h->m, n = h->n, np = p.np;
    const size_t rm = (size_t)p.dr * m, cn = (size_t)p.dc * np;
    std::vector<uint8_t> rdeg((size_t)m, 0);
    std::vector<uint16_t> wcol(rm, (uint16_t)np), wepos(cn, (uint16_t)rm);  // phantom defaults
    std::vector<int32_t> seen((size_t)n, 0);
    for (int i = 0; i < m; ++i) {
        const int lo = h->h_row_ptr[(size_t)i];
        rdeg[(size_t)i] = (uint8_t)(h->h_row_ptr[(size_t)i + 1] - lo);
        for (int e = lo; e < h->h_row_ptr[(size_t)i + 1]; ++e) {
            const int k = e - lo, j = h->h_col_idx[(size_t)e], kc = seen[(size_t)j]++;
            wcol[(size_t)i * p.dr + k] = (uint16_t)j;
            wepos[(size_t)j * p.dc + kc] = (uint16_t)((size_t)i * p.dr + k);
        }
    }
    int rc;
    if ((rc = h->wp_rdeg.ensure(rdeg.size())) || (rc = h->wp_col.ensure(rm * 2)) || (rc = h->wp_epos.ensure(cn * 2))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->wp_rdeg.p, rdeg.data(), rdeg.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->wp_col.p, wcol.data(), rm * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->wp_epos.p, wepos.data(), cn * 2, hipMemcpyHostToDevice));
    h->wave_ps_dr = p.dr;
    h->wave_ps_dc = p.dc;
    return LDPC_HIP_OK;
}

// ---- what the launches of the lane = node and lane = entry kernels share (bp_wave_kernel, bp_wave_ps_kernel, bp_wave_relay_kernel, bp_wave_gd_kernel, bp_wave_f32_kernel, bp_wave_rp_kernel) ----
// PLAN: WavePlan or WavePsPlan (team, waves, groups_per_cu, shared, per_wave, np); ARGS: WaveArgs, WavePsArgs or WaveF32Args, where their field names agree.

// a team per syndrome and no more syndromes than resident teams -- e.g. ONE decode(): static assignment, no work counter to reset
template <class PLAN>
static bool wave_static_teams(const PLAN &p, int64_t batch) { return p.team && batch <= 256 * (int64_t)p.groups_per_cu; }
// workgroups: a team per syndrome or a wavefront per syndrome, no more than are resident
template <class PLAN>
static int64_t wave_groups(const PLAN &p, int64_t batch) {
    const int64_t groups = p.team ? batch : (batch + p.waves - 1) / p.waves, resident = 256 * (int64_t)p.groups_per_cu;
    return groups > resident ? resident : groups;
}

// The work counters, zeroed unless the teams are static.  hook: the block that takes BP + OSD's hand-over where it is armed (the OSD counters sit
// right behind the work pools and share the fill); nullptr: a kernel without one -- bposd_device then lists the unsolved rows itself.
template <class ARGS = WaveArgs>
static int wave_counters(ldpc_hip_bp *h, bool static_teams, ARGS *hook = nullptr) {
    int rc;
    if ((rc = h->counter.ensure(counter_bytes()))) return rc;
    const bool osd_hook = hook && h->osd_hook.armed && h->osd_hook.count == osd_counter_ptr(h);
    if (osd_hook && static_teams) HIPCHK(hipMemsetAsync(osd_counter_ptr(h), 0, OSD_COUNTER_BYTES, h->stream));
    if (!static_teams) HIPCHK(hipMemsetAsync(h->counter.p, 0, osd_hook ? counter_bytes() : work_pool_bytes(), h->stream));
    if (osd_hook) { hook->osd_list = h->osd_hook.list; hook->osd_count = h->osd_hook.count; hook->osd_status = h->osd_hook.status; h->osd_hook.done = true; }
    return LDPC_HIP_OK;
}

// what the argument blocks say of the position tables (ensure_wave_tables, ensure_wave_ps_tables) and what goes with them
static void wave_table_fields(const ldpc_hip_bp *h, const WavePlan &p, WaveArgs &a) {
    a.mp = p.mp;
    a.ms_scaling_factor = h->ms_scaling_factor;
    a.rdeg = (const uint8_t *)h->w_rdeg.p; a.cdeg = (const uint8_t *)h->w_cdeg.p;
    a.col = (const uint16_t *)h->w_col.p; a.apos = (const uint16_t *)h->w_apos.p;
}
static void wave_table_fields(const ldpc_hip_bp *h, const WavePlan &p, WaveF32Args &a) {
    a.mp = p.mp;
    a.ms_scaling_factor = h->ms_scaling_factor;
    a.rdeg = (const uint8_t *)h->w_rdeg.p;
    a.col = (const uint16_t *)h->w_col.p; a.apos = (const uint16_t *)h->w_apos.p;
}
static void wave_table_fields(const ldpc_hip_bp *h, const WavePsPlan &, WavePsArgs &a) {
    a.rdeg = (const uint8_t *)h->wp_rdeg.p; a.col = (const uint16_t *)h->wp_col.p; a.epos = (const uint16_t *)h->wp_epos.p;
    a.min_rdeg = h->m;
    for (int i = 0; i < h->m; ++i) a.min_rdeg = std::min(a.min_rdeg, h->h_row_ptr[(size_t)i + 1] - h->h_row_ptr[(size_t)i]);
}

// The launch.  `args` is the kernel's argument block and `a` the WaveArgs / WavePsArgs in it (the plain kernels: args itself); the caller has ensured the
// position tables, called wave_counters, set the fields that are its kernel's own and launched the kernels that fill its tables.  Here: the fields all
// share, the static share for a handful of syndromes and work_pool_next beyond, the clock probe, LDS above 48 KiB, the grid, the timing events.
template <class KARGS, class ARGS, class PLAN>
static int launch_wave(ldpc_hip_bp *h, const PLAN &p, void (*kern)(const KARGS), KARGS &args, ARGS &a, const DecodeIo &io) {
    const bool static_teams = wave_static_teams(p, io.batch);
    a.pool_per = work_pool_share(io.batch, 0);
    a.m = h->m; a.n = h->n; a.np = p.np; a.max_iter = h->max_iter;
    a.batch = io.batch;
    wave_table_fields(h, p, a);
    a.llr0 = h->d_llr0;
    a.synd = io.synd; a.decoding = io.decoding; a.llr = io.llr; a.iters = io.iters; a.conv = io.conv;
    a.next = static_teams ? nullptr : (unsigned long long *)h->counter.p;
    a.clk = h->d_clk;
    a.lds_shared = (int32_t)p.shared; a.lds_per_wave = (int32_t)p.per_wave;
    const size_t dyn = p.shared + (size_t)(p.team ? 1 : p.waves) * p.per_wave;
    if (dyn > 48u * 1024u)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    const int64_t groups = wave_groups(p, io.batch);
    h->accumulated_ms = 0.f;
    const bool timed = !(h->untimed_call && static_teams);
    // (the timing events ride on the dispatch itself -- hipExtLaunchKernelGGL attaches them to the kernel's own start and completion -- instead of
    // two hipEventRecord around it: those are a barrier packet each on the stream, 5.8 us of a 0.38 ms step, profiles/r6_c5_step_fusion.txt)
    if (timed) LDPC_LAUNCH_TIMED(kern, dim3((unsigned)groups), dim3((unsigned)(p.waves * 64)), (unsigned)dyn, h->stream, h->ev0, h->ev1, 0, args);
    else LDPC_LAUNCH(kern, dim3((unsigned)groups), dim3((unsigned)(p.waves * 64)), (unsigned)dyn, h->stream, args);
    h->timed = timed;
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

static int decode_wave_ps(ldpc_hip_bp *h, const WavePsPlan &p, const DecodeIo &io) {
    int rc;
    WavePsArgs a = {};
    if ((rc = ensure_wave_ps_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch), &a)) || (rc = launch_wave(h, p, p.kern, a, a, io))) return rc;
#ifdef LDPC_WPS_PROF  // measurement build: print and clear the kernel's cycle sums (tools/wave_ps_phases.py)
    {
        HIPCHK(hipStreamSynchronize(h->stream));
        unsigned long long v[12] = {};
        HIPCHK(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_wps_prof), sizeof v));
        fprintf(stderr, "[wps_prof] team %d waves %d groups %lld batch %lld : checkA %llu checkB %llu bitA %llu bitB+synd %llu close %llu setup/out %llu pull %llu iterations %llu syndromes %llu\n",
                (int)p.team, p.waves, (long long)wave_groups(p, io.batch), (long long)io.batch, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
        unsigned long long z[12] = {};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_wps_prof), z, sizeof z));
    }
#endif
    return LDPC_HIP_OK;
}

// Wavefront-per-syndrome on-chip variant (bp_wave_kernel).  Device pointers, on h->stream.
static int decode_wave(ldpc_hip_bp *h, const WavePlan &p, const DecodeIo &io) {
    int rc;
    WaveArgs a = {};
    if ((rc = ensure_wave_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch), &a))) return rc;
    if (p.prior_global) {
        if ((rc = h->w_prior.ensure(sizeof(double) * (size_t)(p.np + 2)))) return rc;
        LDPC_LAUNCH(wave_prior_pad_kernel, dim3((unsigned)((p.np + 2 + 255) / 256)), dim3(256), 0, h->stream, h->d_llr0, h->n, p.np, (double *)h->w_prior.p);
        a.prior_g = (const double *)h->w_prior.p;
    }
    a.llr_direct = p.llr_direct ? 1 : 0;
    return launch_wave(h, p, p.kern, a, a, io);
}

// ---- the lane = edge kernels (min-sum, messages in registers) ----
// One plan for the two families: family 1, bp_edge_kernel -- rows in four lanes: rows <= 4, columns 1 .. 2 entries, 4 m <= 1024 slots; family 2,
// bp_edge8_kernel -- rows in eight lanes: rows <= 8, columns 1 .. 4 entries, 8 m <= 64 R slots.
struct EdgePlan {
    int family = 0;  // 0: not applicable
    int rounds = 0, dc = 0;  // (dc: family 2, the column weight its kernels are built for)
    bool uniform = false;  // every column has the same prior: the form without prior registers (bp_edge_kernel<R, true>, bp_edge8_kernel<R, C, true>)
    bool noclamp = false;  // family 1: ... and the clamp cannot bite (bp_edge_kernel<R, true, true>)
    void (*kern)(const EdgeArgs) = nullptr;    // family 1
    void (*kern8)(const Edge8Args) = nullptr;  // family 2
};

// a column without entries has no lane to write its outputs
static bool every_column_has_an_entry(const ldpc_hip_bp *h) {
    std::vector<char> seen((size_t)h->n, 0);
    for (int32_t j : h->h_col_idx) seen[(size_t)j] = 1;
    for (char c : seen) if (!c) return false;
    return true;
}
// all priors bit-equal?
static bool priors_uniform(const ldpc_hip_bp *h) {
    for (int j = 1; j < h->n; ++j)
        if (std::memcmp(&h->channel_probs[(size_t)j], &h->channel_probs[0], sizeof(double)) != 0) return false;
    return true;
}

static EdgePlan plan_edge(const ldpc_hip_bp *h) {
    EdgePlan p;
    if (h->bp_method != LDPC_HIP_MINIMUM_SUM || h->m <= 0 || h->n <= 0 || h->nnz <= 0) return p;
    if (h->max_row_deg > 4 || h->max_col_deg > 2 || h->n > 65535) return p;
    const int rounds = (4 * h->m + 63) / 64;
    if (rounds > 16 || !every_column_has_an_entry(h)) return p;
#define LDPC_GENERAL(R) bp_edge_kernel<R, false>,
#define LDPC_UNIFORM(R) bp_edge_kernel<R, true>,
#define LDPC_NOCLAMP(R) bp_edge_kernel<R, true, true>,
    static void (*const kerns[3][17])(const EdgeArgs) = {{nullptr, LDPC_EDGE_LADDER(LDPC_GENERAL)}, {nullptr, LDPC_EDGE_LADDER(LDPC_UNIFORM)}, {nullptr, LDPC_EDGE_LADDER(LDPC_NOCLAMP)}};
#undef LDPC_GENERAL
#undef LDPC_UNIFORM
#undef LDPC_NOCLAMP
    p.uniform = priors_uniform(h);
    p.family = 1;
    p.rounds = rounds;
    // the form without the clamp to DBL_MAX (bp_edge_kernel.h, NOCLAMP): finite prior, |alpha| <= 1 (0 = the adaptive 1 - 2^-it), rows of two or more
    bool noclamp = p.uniform && std::isfinite(std::log((1 - h->channel_probs[0]) / h->channel_probs[0])) && std::fabs(h->ms_scaling_factor) <= 1.0 && !h->on("EDGE_CLAMP");
    for (int i = 0; i < h->m && noclamp; ++i) noclamp = h->h_row_ptr[(size_t)i + 1] - h->h_row_ptr[(size_t)i] >= 2;
    p.noclamp = noclamp;
    p.kern = kerns[p.uniform ? (noclamp ? 2 : 1) : 0][rounds];
    return p;
}

__global__ void edge_prior_kernel(const double *llr0, const int32_t *scol, const uint8_t *kind, int slots, double *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < slots) out[s] = kind[s] ? llr0[scol[s]] : __builtin_inf();  // phantom lanes: +inf (bp_edge_kernel.h)
}
// h->d_llr0 per slot into h->e_prior, before every launch that reads it (the priors may have changed since the last call: ldpc_hip_bp_set_channel)
static void launch_edge_prior(ldpc_hip_bp *h, int slots) {
    LDPC_LAUNCH(edge_prior_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, h->d_llr0, (const int32_t *)h->e_scol.p,
                (const uint8_t *)h->e_kind.p, slots, (double *)h->e_prior.p);
}

// the slot tables of either family into e_partner (partner / cpos), e_kind, e_scol, with room for the priors per slot in e_prior; key: h->edge_rounds
static int upload_edge_tables(ldpc_hip_bp *h, int key, const std::vector<uint16_t> &partner, const std::vector<uint8_t> &kind, const std::vector<int32_t> &scol) {
    const size_t slots = kind.size();
    int rc;
    if ((rc = h->e_partner.ensure(partner.size() * 2)) || (rc = h->e_kind.ensure(slots)) || (rc = h->e_scol.ensure(slots * 4)) ||
        (rc = h->e_prior.ensure(slots * 8))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));  // a previous launch may still read the old tables
    HIPCHK(hipMemcpy(h->e_partner.p, partner.data(), partner.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->e_kind.p, kind.data(), slots, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->e_scol.p, scol.data(), slots * 4, hipMemcpyHostToDevice));
    h->edge_rounds = key;
    return LDPC_HIP_OK;
}

// slot tables of bp_edge_kernel: entry k of row i sits in slot 4 i + k (see bp_edge_kernel.h)
static int ensure_edge_tables(ldpc_hip_bp *h, const EdgePlan &p) {
    if (h->edge_rounds == p.rounds) return LDPC_HIP_OK;
    const int slots = p.rounds * 64;
    std::vector<uint16_t> partner((size_t)slots, (uint16_t)(slots + 1));  // phantom lanes read the slot that holds +inf
    std::vector<uint8_t> kind((size_t)slots, 0);
    std::vector<int32_t> scol((size_t)slots, 0), first((size_t)h->n, -1);
    for (int i = 0; i < h->m; ++i)
        for (int e = h->h_row_ptr[(size_t)i]; e < h->h_row_ptr[(size_t)i + 1]; ++e) {
            const int s = 4 * i + (e - h->h_row_ptr[(size_t)i]), j = h->h_col_idx[(size_t)e];
            scol[(size_t)s] = j;
            if (first[(size_t)j] < 0) { first[(size_t)j] = s; kind[(size_t)s] = 1; partner[(size_t)s] = (uint16_t)slots; }  // rows ascend: the column's first entry (bp.hpp:278); alone so far: the +0.0 slot
            else { kind[(size_t)s] = 2; partner[(size_t)s] = (uint16_t)first[(size_t)j]; partner[(size_t)first[(size_t)j]] = (uint16_t)s; }
        }
    return upload_edge_tables(h, p.rounds, partner, kind, scol);
}

static EdgePlan plan_edge8(const ldpc_hip_bp *h) {
    EdgePlan p;
    if (h->bp_method != LDPC_HIP_MINIMUM_SUM || h->m <= 0 || h->n <= 0 || h->nnz <= 0) return p;
    if (h->max_row_deg > 8 || h->max_col_deg > 4 || h->n > 65535) return p;
    const int dc = h->max_col_deg <= 3 ? 3 : 4;
    const int need = (8 * h->m + 63) / 64;
    int rounds = 0;  // the first rung of the column weight (they ascend) that holds the code
#define LDPC_RUNG(R, C) if (dc == C && !rounds && R >= need) rounds = R;
    LDPC_EDGE8_LADDER(LDPC_RUNG)
#undef LDPC_RUNG
    if (!rounds || !every_column_has_an_entry(h)) return p;
    p.uniform = priors_uniform(h);
#define LDPC_E8(R, C) if (rounds == R && dc == C) p.kern8 = p.uniform ? bp_edge8_kernel<R, C, true> : bp_edge8_kernel<R, C, false>;
    LDPC_EDGE8_LADDER(LDPC_E8)
#undef LDPC_E8
    p.family = 2;
    p.rounds = rounds;
    p.dc = dc;
    return p;
}

// slot tables of bp_edge8_kernel: entry k of row i sits in slot 8 i + k (see bp_edge_kernel.h)
static int ensure_edge8_tables(ldpc_hip_bp *h, const EdgePlan &p) {
    const int key = 1000 + p.rounds * 8 + p.dc;
    if (h->edge_rounds == key) return LDPC_HIP_OK;
    const int slots = p.rounds * 64, dc = p.dc;
    std::vector<uint16_t> cpos((size_t)dc * slots, (uint16_t)(slots + 1));  // phantom lanes read the slot that holds +inf
    std::vector<uint8_t> kind((size_t)slots, 0);
    std::vector<int32_t> scol((size_t)slots, slots + 2);  // phantom lanes: the dummy slot
    std::vector<std::vector<int>> col_slots((size_t)h->n);
    for (int i = 0; i < h->m; ++i)
        for (int e = h->h_row_ptr[(size_t)i]; e < h->h_row_ptr[(size_t)i + 1]; ++e) {
            const int s = 8 * i + (e - h->h_row_ptr[(size_t)i]), j = h->h_col_idx[(size_t)e];
            scol[(size_t)s] = j;
            kind[(size_t)s] = (uint8_t)(1 + col_slots[(size_t)j].size());  // rows ascend: the column's order (bp.hpp:278)
            col_slots[(size_t)j].push_back(s);
        }
    for (int j = 0; j < h->n; ++j)
        for (int s : col_slots[(size_t)j])
            for (int q = 0; q < dc; ++q)
                cpos[(size_t)q * slots + s] = (uint16_t)(q < (int)col_slots[(size_t)j].size() ? col_slots[(size_t)j][(size_t)q] : slots);  // beyond the column: +0.0
    return upload_edge_tables(h, key, cpos, kind, scol);
}

// Which lane = edge family takes the handle's code, with its plan: rows in four lanes first, rows in eight lanes (heavier nodes) if that does not
static EdgePlan plan_edge_family(const ldpc_hip_bp *h) {
    const EdgePlan p = plan_edge(h);
    return p.family ? p : plan_edge8(h);
}

// How the lane = edge kernels share a batch among their wavefronts (work_pool_next, bp_device_common.h): one syndrome each to
// start with, the rest in WORK_POOLS slices behind a work counter each.  Syndromes per visit: 1, except for the smallest codes
// (one round: a syndrome takes a few microseconds) on large batches.  EDGE_STATIC_PCT / EDGE_CHUNK: measurement overrides.
template <typename ARGS>
static int edge_work_split(ldpc_hip_bp *h, int rounds, int64_t batch, int64_t groups, ARGS &a) {
    int rc;
    if ((rc = h->counter.ensure(counter_bytes()))) return rc;
    HIPCHK(hipMemsetAsync(h->counter.p, 0, work_pool_bytes(), h->stream));
    a.next = (unsigned long long *)h->counter.p;
    a.clk = h->d_clk;
    int64_t static_per = 1;
    if (h->sw("EDGE_STATIC_PCT") >= 0) static_per = (batch * (h->sw("EDGE_STATIC_PCT") > 100 ? 100 : h->sw("EDGE_STATIC_PCT")) / 100) / groups;
    a.static_per = (int32_t)static_per;
    a.dyn_base = (int32_t)(static_per * groups);
    a.pool_per = work_pool_share(batch, a.dyn_base);
    int64_t c = rounds >= 2 ? 1 : batch / (groups * 16);
    if (h->sw("EDGE_CHUNK") > 0) c = h->sw("EDGE_CHUNK");
    a.chunk = (int32_t)(c < 1 ? 1 : c > 8 ? 8 : c);
    return LDPC_HIP_OK;
}

// The two families differ for the host in two things, said here once: which slot tables a plan asks for, and which field of the inner argument block --
// the EdgeArgs / Edge8Args / EdgeF32Args / Edge8F32Args, which the plain kernels take as it is and the variants carry as `e` -- points at e_partner.
static EdgeArgs &edge_inner(EdgeArgs &a) { return a; }
static Edge8Args &edge_inner(Edge8Args &a) { return a; }
static EdgeF32Args &edge_inner(EdgeF32Args &a) { return a; }
static Edge8F32Args &edge_inner(Edge8F32Args &a) { return a; }
template <class KARGS> static auto edge_inner(KARGS &args) -> decltype((args.e)) { return args.e; }
static const uint16_t *&edge_partner_field(EdgeArgs &e) { return e.partner; }
static const uint16_t *&edge_partner_field(Edge8Args &e) { return e.cpos; }
static const uint16_t *&edge_partner_field(EdgeF32Args &e) { return e.partner; }
static const uint16_t *&edge_partner_field(Edge8F32Args &e) { return e.cpos; }
// the first step of every lane = edge mode: the plan's slot tables, and `args` told where they are
template <class KARGS>
static int edge_tables(ldpc_hip_bp *h, const EdgePlan &p, KARGS &args) {
    const int rc = p.family == 1 ? ensure_edge_tables(h, p) : ensure_edge8_tables(h, p);
    if (rc) return rc;
    edge_partner_field(edge_inner(args)) = (const uint16_t *)h->e_partner.p;
    return LDPC_HIP_OK;
}

// The launch of EVERY lane = edge kernel -- FP64 and FP32, rows in four and in eight lanes, plain, row priors, memory, Relay-BP, decimation.  `args` is
// the kernel's argument block; the mode has called edge_tables, set what is its own in it -- the priors, a variant's tables -- and launched the kernels
// that fill them.  Here: the fields all share, one wavefront per workgroup and as many of them resident as LDS (`dyn` bytes and the kernels' few static
// ones, of 160 KiB) and the registers (the wavefronts per SIMD the instantiation was compiled for) allow, the work split, the launch between the two
// timing events.
template <class KARGS>
static int launch_edge(ldpc_hip_bp *h, void (*kern)(const KARGS), KARGS &args, int rounds, size_t dyn, int waves_per_simd, const DecodeIo &io) {
    auto &a = edge_inner(args);
    a.m = h->m; a.n = h->n; a.max_iter = h->max_iter;
    a.ms_scaling_factor = h->ms_scaling_factor;
    a.batch = io.batch;
    a.kind = (const uint8_t *)h->e_kind.p; a.scol = (const int32_t *)h->e_scol.p;
    a.synd = io.synd; a.decoding = io.decoding; a.llr = io.llr; a.iters = io.iters; a.conv = io.conv;
    int64_t per_cu = (int64_t)((160u * 1024u) / (dyn + 64));
    if (per_cu > 4 * (int64_t)waves_per_simd) per_cu = 4 * (int64_t)waves_per_simd;
    const int64_t groups = io.batch < 256 * per_cu ? io.batch : 256 * per_cu;
    int rc;
    if ((rc = edge_work_split(h, rounds, io.batch, groups, a))) return rc;
    h->accumulated_ms = 0.f;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    LDPC_LAUNCH(kern, dim3((unsigned)groups), dim3(64), (unsigned)dyn, h->stream, args);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// a zeroed argument block of the type `kern` takes
template <class KARGS> static KARGS kernel_args(void (*)(const KARGS)) { return {}; }

// Each mode below is one function: `launch` is its body, written once for the argument blocks of both families, and its last line hands `launch` the
// family's kernel and the wavefronts per SIMD that kernel was compiled for.
static int decode_edge(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern) -> int {
        auto a = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, a))) return rc;
        launch_edge_prior(h, p.rounds * 64);
        a.prior_s = (const double *)h->e_prior.p;
        a.prior_u = std::log((1 - h->channel_probs[0]) / h->channel_probs[0]);  // as upload_priors (bp.hpp:150-151); read by the uniform form only
        return launch_edge(h, kern, a, p.rounds, edge_lds_bytes(p.rounds), p.uniform ? 5 : 4, io);  // (__launch_bounds__(64, UNIFORM ? 5 : 4))
    };
    return p.family == 1 ? launch(p.kern) : launch(p.kern8);
}

// ---- the same two families with FP32 messages (bp_edge_f32_kernel.h; instantiated in tu_onchip_f32.hip): the float32 message mode's on-chip route ----
// One plan answers for both dtypes (plan_edge, plan_edge8) and the slot tables are shared (ensure_edge_tables, ensure_edge8_tables, keyed by
// h->edge_rounds).  e_prior is rewritten before every launch, here as floats, there as doubles, on the same stream: a handle that
// changes its message dtype never reads one type's priors as the other's.
__global__ void edge_prior_f32_kernel(const double *llr0, const int32_t *scol, const uint8_t *kind, int slots, float *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < slots) out[s] = kind[s] ? (float)llr0[scol[s]] : __builtin_inff();  // one rounding (v_cvt_f32_f64); phantom lanes: +inf
}

static int decode_edge_f32(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern, int waves_per_simd) -> int {
        auto a = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, a))) return rc;
        if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "float32 messages: no on-chip kernel was built for %d rounds", p.rounds);
        const int slots = p.rounds * 64;
        LDPC_LAUNCH(edge_prior_f32_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, h->d_llr0, (const int32_t *)h->e_scol.p,
                    (const uint8_t *)h->e_kind.p, slots, (float *)h->e_prior.p);
        a.prior_s = (const float *)h->e_prior.p;
        a.prior_u = (float)std::log((1 - h->channel_probs[0]) / h->channel_probs[0]);  // the FP64 prior of upload_priors, rounded once; read by the uniform form only
        return launch_edge(h, kern, a, p.rounds, edge_f32_lds_bytes(p.rounds), waves_per_simd, io);
    };
    return p.family == 1 ? launch(edge_f32_kernel(p.rounds, p.uniform, p.noclamp), edge_f32_waves(p.rounds))
                         : launch(edge8_f32_kernel(p.rounds, p.dc, p.uniform), edge8_f32_waves(p.rounds, p.dc, p.uniform));
}

// ---- the same two families with row priors (bp_edge_rp_kernel.h; instantiated in tu_onchip_rp.hip): ldpc_hip_*_decode_batch_priors on the codes of plan_edge / plan_edge8 ----
// The priors: h->row_probs [batch][n] -> h->rowp_llr [batch][n] log-ratios, whole batch (row_priors_rowmajor_kernel, io_kernels.h); e_prior is neither
// written nor read, so the next plain call finds it as its own last launch left it (and rewrites it anyway).
static int decode_edge_rp(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern) -> int {
        auto ra = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, ra))) return rc;
        if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "row priors: no lane = edge kernel was built for %d rounds", p.rounds);
        const size_t items = (size_t)io.batch * (size_t)h->n;
        if ((rc = h->rowp_llr.ensure(sizeof(double) * items))) return rc;
        LDPC_LAUNCH(row_priors_rowmajor_kernel, flat_grid(items), dim3(256), 0, h->stream, h->row_probs, (int64_t)items, (double *)h->rowp_llr.p);
        HIPCHK(hipGetLastError());
        ra.rowp = (const double *)h->rowp_llr.p;
        return launch_edge(h, kern, ra, p.rounds, edge_lds_bytes(p.rounds), 4, io);  // (__launch_bounds__(64, 4): the general form's four wavefronts per SIMD)
    };
    return p.family == 1 ? launch(edge_rp_kernel(p.rounds)) : launch(edge8_rp_kernel(p.rounds, p.dc));
}

// Row priors on the lane = edge kernels?  Debug switch EDGE_RP: 0 the slot kernel (bp_small_kernel<., ., true>), 1 bp_edge_rp_kernel /
// bp_edge8_rp_kernel, unset: the default below -- the route, by the rule fixed before it was measured: on one MI355X in one
// job it beat the slot kernel, the parent's row-prior decode, 3.1x on BB144 min-sum 50 (87.1 against 27.8 M syndromes/s) and 17.2x on the
// surface code d = 21 min-sum 30 (43.7 against 2.54 M/s), the parent's two runs 0.3 % and 0.5 % apart (profiles/row_priors_edge.jsonl).
static constexpr bool k_edge_rp_default = true;
static bool edge_rp_route(const ldpc_hip_bp *h) {
    const int s = h->sw("EDGE_RP");
    return s >= 0 ? s != 0 : k_edge_rp_default;
}

// ---- the same two families with memory (bp_edge_mem_kernel.h; instantiated in tu_onchip_mem.hip): ldpc_hip_bp_set_memory on the codes of plan_edge / plan_edge8 ----
// e_prior (the log-ratios per slot) holds the initial messages, as in the plain decode.  The memory: a[] and gamma[] of the handle (mem_ag,
// upload_memory) per slot into e_mem, before every launch as e_prior is -- the priors or the strengths may have changed since the last one.
__global__ void edge_mem_table_kernel(const double *ag, int n, const int32_t *scol, const uint8_t *kind, int slots, double *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    out[s] = kind[s] ? ag[scol[s]] : __builtin_inf();   // phantom lanes: prior +inf for good ...
    out[slots + s] = kind[s] ? ag[n + scol[s]] : 0.0;   // ... by strength 0 (bp_edge_mem_kernel.h)
}

static int decode_edge_mem(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern, int waves_per_simd) -> int {
        auto ma = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, ma))) return rc;
        if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "memory min-sum: no lane = edge kernel was built for %d rounds", p.rounds);
        const int slots = p.rounds * 64;
        if ((rc = h->e_mem.ensure(sizeof(double) * 2 * (size_t)slots))) return rc;
        launch_edge_prior(h, slots);
        LDPC_LAUNCH(edge_mem_table_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->mem_ag.p, h->n, (const int32_t *)h->e_scol.p,
                    (const uint8_t *)h->e_kind.p, slots, (double *)h->e_mem.p);
        HIPCHK(hipGetLastError());
        ma.a_s = (const double *)h->e_mem.p;
        ma.g_s = (const double *)h->e_mem.p + slots;
        ma.e.prior_s = (const double *)h->e_prior.p;
        return launch_edge(h, kern, ma, p.rounds, edge_lds_bytes(p.rounds), waves_per_simd, io);
    };
    return p.family == 1 ? launch(edge_mem_kernel(p.rounds), edge_mem_waves(p.rounds)) : launch(edge8_mem_kernel(p.rounds, p.dc), edge8_mem_waves(p.rounds, p.dc));
}

// ---- the same two families as Relay-BP (bp_edge_relay_kernel.h; instantiated in tu_onchip_relay.hip): ldpc_hip_bp_set_relay on the codes of plan_edge / plan_edge8 ----
// As the memory decode, except that the slot tables of a and gamma are per leg: relay_ag [legs][2][n] (upload_relay) -> e_relay [legs][2][R * 64],
// before every launch.
__global__ void edge_relay_table_kernel(const double *ag, int n, int legs, const int32_t *scol, const uint8_t *kind, int slots, double *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    const bool real = kind[s] != 0;
    const int j = real ? scol[s] : 0;
    for (int l = 0; l < legs; ++l) {
        out[(size_t)l * 2 * slots + s] = real ? ag[(size_t)l * 2 * n + j] : __builtin_inf();    // phantom lanes: prior +inf for good ...
        out[(size_t)l * 2 * slots + slots + s] = real ? ag[(size_t)l * 2 * n + n + j] : 0.0;    // ... by strength 0
    }
}

static int decode_edge_relay(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern, int waves_per_simd) -> int {
        auto ma = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, ma))) return rc;
        if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "Relay-BP: no lane = edge kernel was built for %d rounds", p.rounds);
        const int slots = p.rounds * 64;
        if ((rc = h->e_relay.ensure(sizeof(double) * 2 * (size_t)slots * (size_t)h->relay_legs))) return rc;
        launch_edge_prior(h, slots);
        LDPC_LAUNCH(edge_relay_table_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->relay_ag.p, h->n, h->relay_legs,
                    (const int32_t *)h->e_scol.p, (const uint8_t *)h->e_kind.p, slots, (double *)h->e_relay.p);
        HIPCHK(hipGetLastError());
        ma.ag_s = (const double *)h->e_relay.p;
        ma.leg_iters = (const int32_t *)h->relay_it.p;
        ma.llr0 = h->d_llr0;
        ma.legs = h->relay_legs; ma.stop_after = h->relay_stop;
        ma.e.prior_s = (const double *)h->e_prior.p;
        return launch_edge(h, kern, ma, p.rounds, edge_lds_bytes(p.rounds), waves_per_simd, io);  // (e.max_iter is not read: leg_iters takes its place)
    };
    return p.family == 1 ? launch(edge_relay_kernel(p.rounds), edge_relay_waves(p.rounds)) : launch(edge8_relay_kernel(p.rounds, p.dc), edge8_relay_waves(p.rounds, p.dc));
}

// ---- Relay-BP and memory min-sum on the lane = node kernel (bp_wave_relay_kernel.h; instantiated in tu_onchip_wave_relay.hip): the codes beyond both lane = edge ladders ----
// plan_wave's shared rules (the ladder, wave_pad, wave_padding_dominates, wave_team_rule and what follows it), min-sum only, the priors always read from
// the padded device array, and the wavefronts capped by what the instantiation was compiled for.  waves == 0: not applicable.  One planner for this
// kernel, for bp_wave_gd_kernel (plan_wave_gd), for bp_wave_f32_kernel (plan_wave_f32) and for bp_wave_rp_kernel (plan_wave_rp): what differs between them is said in a WaveLdsKernel --
// the LDS sizes, the wavefronts its instantiations are compiled for, the wavefronts per compute
// unit its registers allow -- and, where the kernel has the two forms of bp_wave_kernel's log-ratios, the size without the LDS copy.
// (It stays a planner of its own beside plan_wave: the two share the rules above, but plan_wave chooses its kernel and prior_global, and has
// other caps and another refusal -- merged, every second line would ask which of the two it serves.)
struct WaveLdsKernel {
    size_t (*lds_shared)(int mp, int np, int dr, int dc);
    size_t (*lds_private)(int mp, int np, int dr);       // a syndrome's private region (with the posteriors in LDS where the kernel keeps them there)
    size_t (*lds_private_lean)(int mp, int np, int dr);  // ... without the copy of the posteriors: the llr_direct form; nullptr: the kernel has none
    int (*waves)(int dr, int dc, bool team);             // wave_ms_waves / wave_f32_waves
    int solo_cap;                                        // wavefronts per compute unit, one syndrome each
};
// llr_form (kernels with a lean form only): -1 wave_llr_direct_rule decides, 0 the LDS copy, 1 llr_direct.  lds_static: the bytes left free for the
// kernel's static LDS -- WAVE_RELAY_LDS_STATIC / WAVE_GD_LDS_STATIC / WAVE_F32_LDS_STATIC / WAVE_RP_LDS_STATIC, which each kernel asserts it keeps to.
static WavePlan plan_wave_lds(const ldpc_hip_bp *h, bool forced, int64_t batch, const WaveLdsKernel &k, int llr_form, size_t lds_static) {
    WavePlan p;
    if (h->bp_method != LDPC_HIP_MINIMUM_SUM || h->m <= 0 || h->n <= 0 || h->nnz <= 0 || h->max_row_deg > 16 || h->max_col_deg > 8) return p;
#define LDPC_RUNG(R, C) if (!p.dr && h->max_row_deg <= R && h->max_col_deg <= C) { p.dr = R; p.dc = C; }
    LDPC_WAVE_LADDER(LDPC_RUNG)
#undef LDPC_RUNG
    if (!wave_pad(h, p) || (!forced && wave_padding_dominates(h, p))) return p;
    p.shared = k.lds_shared(p.mp, p.np, p.dr, p.dc);
    p.per_wave = k.lds_private(p.mp, p.np, p.dr);
    p.prior_global = true;
    const size_t lds = 160u * 1024u - lds_static;  // (the kernel's static LDS comes on top of the dynamic part)
    if (k.lds_private_lean) {
        const size_t lean = k.lds_private_lean(p.mp, p.np, p.dr);
        if (llr_form < 0 ? wave_llr_direct_rule(lds, p.shared, p.per_wave, lean) : llr_form != 0) { p.per_wave = lean; p.llr_direct = true; }
    }
    if (p.shared + p.per_wave > lds) return p;
    size_t w = (lds - p.shared) / p.per_wave;
    if (w > (size_t)k.waves(p.dr, p.dc, false)) w = (size_t)k.waves(p.dr, p.dc, false);
    const int u = wave_ms_nodes_per_lane(p.dr, 1);  // (the row part, as plan_wave)
    if (wave_team_rule(h, p, w, u, batch)) {
        p.team = true;
        p.waves = wave_team_width(p, u, k.waves(p.dr, p.dc, true));
        wave_team_groups(p, lds);
        return p;
    }
    if (!forced && w < 2) return p;
    p.waves = (int)w;
    wave_solo_groups(p, lds, k.solo_cap);
    return p;
}
// (solo_cap 16: the kernels' 87 .. 150 VGPRs allow 16 wavefronts per compute unit, 12 where compiled for 12)
static WavePlan plan_wave_relay(const ldpc_hip_bp *h, bool forced, int64_t batch) {
    static const WaveLdsKernel k = {wave_relay_lds_shared, [](int mp, int np, int dr) { return wave_relay_lds_private(mp, np, dr); }, nullptr, wave_ms_waves, 16};
    return plan_wave_lds(h, forced, batch, k, -1, WAVE_RELAY_LDS_STATIC);
}
// Guided decimation on bp_wave_gd_kernel (bp_wave_gd_kernel.h): the shared tables are the relay kernel's, the private region carries the two masks
static WavePlan plan_wave_gd(const ldpc_hip_bp *h, bool forced, int64_t batch) {
    static const WaveLdsKernel k = {wave_relay_lds_shared, [](int mp, int np, int dr) { return wave_gd_lds_private(mp, np, dr); }, nullptr, wave_ms_waves, 16};
    return plan_wave_lds(h, forced, batch, k, -1, WAVE_GD_LDS_STATIC);
}
// The float32 message mode on bp_wave_f32_kernel (bp_wave_f32_kernel.h): plan_wave's choice between the LDS copy of the log-ratios and llr_direct, with
// the FP32 sizes (debug switch F32_WAVE_LLR: 0 the copy, 1 direct, unset the rule); without log-ratios the lean region is all there is.
// (solo_cap 20: the instantiations' <= 96 VGPRs allow five wavefronts per SIMD)
static WavePlan plan_wave_f32(const ldpc_hip_bp *h, bool forced, bool want_llr, int64_t batch) {
    static const auto copy = [](int mp, int np, int dr) { return wave_f32_lds_private(mp, np, dr, true); };
    static const auto lean = [](int mp, int np, int dr) { return wave_f32_lds_private(mp, np, dr, false); };
    static const WaveLdsKernel with_llr = {wave_f32_lds_shared, copy, lean, wave_f32_waves, 20};
    static const WaveLdsKernel without = {wave_f32_lds_shared, lean, nullptr, wave_f32_waves, 20};
    return plan_wave_lds(h, forced, batch, want_llr ? with_llr : without, h->sw("F32_WAVE_LLR"), WAVE_F32_LDS_STATIC);
}

// a and gamma of every leg as the kernel reads them: [legs][2][np], beyond n a = 1.0 and gamma = 0 (the padding columns form the finite prior 1.0)
__global__ void wave_relay_table_kernel(const double *ag, int n, int np, int legs, double *out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= np) return;
    for (int l = 0; l < legs; ++l) {
        out[(size_t)l * 2 * np + q] = q < n ? ag[(size_t)l * 2 * n + q] : 1.0;
        out[(size_t)l * 2 * np + np + q] = q < n ? ag[(size_t)l * 2 * n + n + q] : 0.0;
    }
}

// ag [legs][2][n]: relay_ag, or mem_ag as one leg (leg_iters == nullptr: to h->max_iter).  No OSD hook: bposd_device lists the unsolved rows itself, as
// after the lane = edge relay kernels.
static int decode_wave_relay(ldpc_hip_bp *h, const WavePlan &p, const double *ag, int legs, const int32_t *leg_iters, int stop_after, const DecodeIo &io) {
    const WaveRelayKernel kern = wave_relay_kernel(p.dr, p.dc, p.team);
    if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "Relay-BP / memory min-sum: no lane = node kernel was built for rows of %d, columns of %d", p.dr, p.dc);
    int rc;
    if ((rc = ensure_wave_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch)))) return rc;
    // w_relay: [np + 2] the padded priors, then [legs][2][np] the padded tables (its own buffer: it goes when the relay or the memory is switched off)
    if ((rc = h->w_relay.ensure(sizeof(double) * ((size_t)(p.np + 2) + 2 * (size_t)p.np * (size_t)legs)))) return rc;
    double *const prior_p = (double *)h->w_relay.p, *const ag_p = prior_p + p.np + 2;
    // (the priors, the strengths or the legs may have changed since the last call)
    LDPC_LAUNCH(wave_prior_pad_kernel, dim3((unsigned)((p.np + 2 + 255) / 256)), dim3(256), 0, h->stream, h->d_llr0, h->n, p.np, prior_p);
    LDPC_LAUNCH(wave_relay_table_kernel, dim3((unsigned)((p.np + 255) / 256)), dim3(256), 0, h->stream, ag, h->n, p.np, legs, ag_p);
    HIPCHK(hipGetLastError());
    WaveRelayArgs ra = {};
    ra.w.prior_g = prior_p;
    ra.ag_p = ag_p;
    ra.leg_iters = leg_iters;
    ra.legs = legs; ra.stop_after = stop_after;
    return launch_wave(h, p, kern, ra, ra.w, io);
}

// Guided decimation on the lane = node kernel (bp_wave_gd_kernel.h; instantiated in tu_onchip_wave_gd.hip): as decode_wave_relay, with the
// padded priors alone in w_gd (written before every launch: the priors may have changed) and the rounds where the relay has its legs.
static int decode_wave_gd(ldpc_hip_bp *h, const WavePlan &p, const DecodeIo &io) {
    const WaveGdKernel kern = wave_gd_kernel(p.dr, p.dc, p.team);
    if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "guided decimation: no lane = node kernel was built for rows of %d, columns of %d", p.dr, p.dc);
    int rc;
    if ((rc = ensure_wave_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch)))) return rc;
    if ((rc = h->w_gd.ensure(sizeof(double) * (size_t)(p.np + 2)))) return rc;
    LDPC_LAUNCH(wave_prior_pad_kernel, dim3((unsigned)((p.np + 2 + 255) / 256)), dim3(256), 0, h->stream, h->d_llr0, h->n, p.np, (double *)h->w_gd.p);
    HIPCHK(hipGetLastError());
    WaveGdArgs ga = {};
    ga.w.prior_g = (const double *)h->w_gd.p;
    ga.freeze_llr = h->gd_freeze;
    ga.round_iters = h->gd_round_iters; ga.max_rounds = h->gd_max_rounds;
    return launch_wave(h, p, kern, ga, ga.w, io);  // (w.max_iter is not read: the rounds take its place)
}

// Is the lane = node route what the default modes (-1, 1) take?  By the rule of DESIGN.md section 7d, stated there before the measurement: the
// default only if it beats the per-pass route by more than the run-to-run spread of the two on both measured codes.  It does, on one MI355X in one
// job (profiles/relay_wave.jsonl): Relay-BP 48.1x on the [[1600,64]] hypergraph product and 48.8x on HGP [[400,16]] (7.64 against 0.159 and 30.4
// against 0.622 M syndromes/s, spreads <= 2.1 %), the memory decode 12.4x and 17.5x (spreads <= 0.15 %).  false: modes 3 / 4 / 5 only.
static constexpr bool k_wave_relay_default = true;

// Which route a Relay-BP or memory decode of `batch` syndromes takes -- one decision for decode_onchip_relay, the memory branch of decode_onchip
// and ldpc_hip_bp_relay_route: 0 the per-pass kernels (the relay's leg loop), 1 bp_edge, 2 bp_edge8, 3 / 4 bp_wave_relay with one wavefront / a team
// per syndrome.  small_mode: 0 everything per pass; 6 stops after the lane = edge families; 4 and 5 force the one-wavefront and the team form, 3 takes
// the plan's own choice; -1 and 1 take it where k_wave_relay_default says so.
// (OnchipRoute: this decision's and plan_gd_route's answer -- the route with the plan that goes with it: ep for 1 and 2, wp for 3 and 4.)
struct OnchipRoute { int route = 0; EdgePlan ep; WavePlan wp; };
static OnchipRoute plan_relay_route(const ldpc_hip_bp *h, int64_t batch) {
    OnchipRoute r;
    if (!(h->small_mode != 0 && onchip_bound(h, batch))) return r;
    r.ep = plan_edge_family(h);
    r.route = r.ep.family;
    if (r.route) return r;
    const bool asked = h->small_mode >= 3 && h->small_mode <= 5;
    if (!asked && !(k_wave_relay_default && (h->small_mode == -1 || h->small_mode == 1))) return r;
    r.wp = plan_wave_relay(h, asked || h->small_mode == 1, batch);
    if (r.wp.waves) r.route = r.wp.team ? 4 : 3;
    return r;
}

int ldpc_hip_bp_relay_route(const ldpc_hip_bp *h, int64_t batch, int32_t *route) {
    if (!h || !route) return fail(LDPC_HIP_ERR_INVALID, "null argument");
    if (batch < 0) return fail(LDPC_HIP_ERR_INVALID, "negative batch");
    if (h->variant != Variant::Relay && h->variant != Variant::Memory) return fail(LDPC_HIP_ERR_INVALID, "neither Relay-BP nor memory min-sum is on (ldpc_hip_bp_set_relay, ldpc_hip_bp_set_memory)");
    *route = plan_relay_route(h, batch).route;
    return LDPC_HIP_OK;
}

// Relay-BP on chip: plan_edge, plan_edge8, plan_wave_relay in that order (plan_relay_route).  *took = false: the per-pass leg loop (host_stream.h: decode_relay).
int decode_onchip_relay(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took) {
    *took = false;
    const DecodeIo io = {synd, batch, decoding, llr, iters, conv};
    const OnchipRoute r = plan_relay_route(h, batch);
    *took = r.route != 0;
    if (r.route == 1 || r.route == 2) return decode_edge_relay(h, r.ep, io);
    if (r.route >= 3) return decode_wave_relay(h, r.wp, (const double *)h->relay_ag.p, h->relay_legs, (const int32_t *)h->relay_it.p, h->relay_stop, io);
    return LDPC_HIP_OK;
}

// ---- the same two families with guided decimation (bp_edge_gd_kernel.h; instantiated in tu_onchip_gd.hip): ldpc_hip_bp_set_decimation on the codes of plan_edge / plan_edge8 ----
// e_prior (L0 per slot) is the plain decode's: every syndrome's priors, initial messages and frozen slots start from it.  The kernels read round_iters and
// max_rounds where the others read max_iter.
// The route: decode_onchip's small-mode rule for the lane = edge families (modes -1, 1, 6), onchip_bound and plan_edge_family.
// With ldpc_hip_bp_set_decimation_lane_node on (opt-in, off by default) the order is plan_relay_route's: any mode but 0 asks plan_edge and plan_edge8, mode
// 6 stops there, and modes -1, 1, 3, 4, 5 go on to plan_wave_gd -- bp_wave_gd_kernel (bp_wave_gd_kernel.h) with one wavefront (3) or a team (4) per
// syndrome, 4 and 5 forcing either.  A per-pass route is not built.
static OnchipRoute plan_gd_route(const ldpc_hip_bp *h, int64_t batch) {
    OnchipRoute r;
    if (!(h->gd_lane_node ? h->small_mode != 0 : h->small_mode == -1 || h->small_mode == 1 || h->small_mode == 6)) return r;
    if (!onchip_bound(h, batch)) return r;
    r.ep = plan_edge_family(h);
    r.route = r.ep.family;
    if (r.route) return r;
    if (!h->gd_lane_node || h->small_mode == 6 || h->small_mode == 2) return r;
    r.wp = plan_wave_gd(h, h->small_mode != -1, batch);  // (forced: as plan_relay_route, by modes 1, 3, 4, 5)
    if (r.wp.waves) r.route = r.wp.team ? 4 : 3;
    return r;
}

// The route alone, for the refusal checks of every entry point and for ldpc_hip_bp_decimation_route: the plans' answer for the handle's code, kept per
// (bp_method, small-code kernel mode) -- nothing else it depends on can change on a handle -- and the batch bound.  (decode_onchip_gd plans once per decode,
// as decode_onchip does: it needs the plans' kernels.)
int gd_route(const ldpc_hip_bp *h, int64_t batch) {
    if (h->gd_route_known < 0 || h->gd_route_method != h->bp_method || h->gd_route_mode != h->small_mode) {
        h->gd_route_known = plan_gd_route(h, 0).route;  // (a batch of 0: whether the lane = node kernel takes the code at all does not depend on it, only 3 or 4 does)
        h->gd_route_method = h->bp_method;
        h->gd_route_mode = h->small_mode;
    }
    if (batch >= (1ll << 30)) return 0;
    if (h->gd_route_known < 3 || batch == 0) return h->gd_route_known;
    return plan_wave_gd(h, h->small_mode != -1, batch).team ? 4 : 3;  // (one wavefront or a team: by the batch; the plan does not scan the matrix)
}

int ldpc_hip_bp_decimation_route(const ldpc_hip_bp *h, int64_t batch, int32_t *route) {
    if (!h || !route) return fail(LDPC_HIP_ERR_INVALID, "null argument");
    if (batch < 0) return fail(LDPC_HIP_ERR_INVALID, "negative batch");
    if (h->variant != Variant::Decimation) return fail(LDPC_HIP_ERR_INVALID, "guided decimation is not on (ldpc_hip_bp_set_decimation)");
    *route = gd_route(h, batch);
    return LDPC_HIP_OK;
}

static int decode_edge_gd(ldpc_hip_bp *h, const EdgePlan &p, const DecodeIo &io) {
    const auto launch = [&](auto kern, int waves_per_simd) -> int {
        auto ga = kernel_args(kern);
        int rc;
        if ((rc = edge_tables(h, p, ga))) return rc;
        if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "guided decimation: no lane = edge kernel was built for %d rounds", p.rounds);
        launch_edge_prior(h, p.rounds * 64);
        ga.e.prior_s = (const double *)h->e_prior.p;
        ga.freeze_llr = h->gd_freeze;
        ga.round_iters = h->gd_round_iters; ga.max_rounds = h->gd_max_rounds;
        return launch_edge(h, kern, ga, p.rounds, edge_lds_bytes(p.rounds), waves_per_simd, io);  // (e.max_iter is not read: the rounds take its place)
    };
    return p.family == 1 ? launch(edge_gd_kernel(p.rounds), edge_gd_waves(p.rounds)) : launch(edge8_gd_kernel(p.rounds, p.dc), edge8_gd_waves(p.rounds, p.dc));
}

int decode_onchip_gd(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv) {
    const DecodeIo io = {synd, batch, decoding, llr, iters, conv};
    const OnchipRoute r = plan_gd_route(h, batch);
    if (r.route == 1 || r.route == 2) return decode_edge_gd(h, r.ep, io);
    if (r.route >= 3) return decode_wave_gd(h, r.wp, io);
    // (decode_gate has said so for the code and the mode; what is left is the batch)
    if (h->gd_lane_node)
        return fail(LDPC_HIP_ERR_UNSUPPORTED, "guided decimation: no on-chip kernel takes a batch of %lld syndromes of this code (ldpc_hip_bp_decimation_route answers 0); "
                    "a per-pass route is not built", (long long)batch);
    return fail(LDPC_HIP_ERR_UNSUPPORTED, "guided decimation: no lane = edge kernel takes a batch of %lld syndromes of this code (ldpc_hip_bp_decimation_route answers 0); "
                "the lane = node route and a per-pass route are not built yet", (long long)batch);
}

// ---- the float32 message mode on the lane = node kernel (bp_wave_f32_kernel.h; instantiated in tu_onchip_wave_f32.hip): the codes beyond both lane = edge ladders, opt-in ----
// As decode_wave_gd: the shared position tables, the work counters without an OSD hook (bposd_device lists the unsolved rows itself), and the padded
// priors -- here floats, in w_prior_f32, written before every launch (the priors may have changed): a buffer of this route alone, so a handle that
// changes its message dtype never reads one type's priors as the other's.
static int decode_wave_f32(ldpc_hip_bp *h, const WavePlan &p, const DecodeIo &io) {
    const WaveF32Kernel kern = wave_f32_kernel(p.dr, p.dc, p.team);
    if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "float32 messages: no lane = node kernel was built for rows of %d, columns of %d", p.dr, p.dc);
    int rc;
    if ((rc = ensure_wave_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch)))) return rc;
    if ((rc = h->w_prior_f32.ensure(sizeof(float) * (size_t)(p.np + 2)))) return rc;
    const WaveF32PriorKernel pad = wave_f32_prior_kernel();
    LDPC_LAUNCH(pad, dim3((unsigned)((p.np + 2 + 255) / 256)), dim3(256), 0, h->stream, (const double *)h->d_llr0, h->n, p.np, (float *)h->w_prior_f32.p);
    HIPCHK(hipGetLastError());
    WaveF32Args a = {};
    a.prior_g = (const float *)h->w_prior_f32.p;
    a.llr_direct = p.llr_direct ? 1 : 0;
    return launch_wave(h, p, kern, a, a, io);
}

// Which route a float32 decode of `batch` syndromes takes -- one decision for decode_onchip_f32 and ldpc_hip_bp_f32_route: 0 the per-pass kernels
// (host_f32.h), 1 bp_edge, 2 bp_edge8 (bp_edge_f32_kernel.h), 3 / 4 bp_wave_f32 with one wavefront / a team per syndrome.
// Per-pass whatever the code: small_mode 0 (never an on-chip kernel) and 2 (the slot kernel, which float32 has none of), the switch F32_ONCHIP 0, and
// any switch that names the per-pass kernels (F32_NT, F32_GRID_ROWS, SPREAD_NODES: who sets one wants those kernels, on whatever code).  Modes -1, 1
// and 6 ask the lane = edge families.  That is all with f32_lane_node off (in float32 nothing then goes beyond the lane = edge kernels).  With it on
// (ldpc_hip_bp_set_f32_lane_node) the order is plan_relay_route's: mode 6 stops after the lane = edge families, modes -1, 1 and 3 take
// plan_wave_f32's own choice between one wavefront and a team (1 and 3 forced, as plan_wave's `forced`), 4 and 5 force either.  No float32 decode
// ever goes to bp_wave_kernel, bp_small_kernel or any FP64 kernel.
static OnchipRoute plan_f32_route(const ldpc_hip_bp *h, int64_t batch, bool want_llr) {
    OnchipRoute r;
    if (h->small_mode == 0 || h->small_mode == 2 || h->sw("F32_ONCHIP") == 0 || h->sw("F32_NT") >= 0 || h->sw("F32_GRID_ROWS") > 0 || h->sw("SPREAD_NODES") > 0) return r;
    if (!onchip_bound(h, batch)) return r;
    if (h->small_mode == -1 || h->small_mode == 1 || h->small_mode == 6) {
        r.ep = plan_edge_family(h);
        r.route = r.ep.family;
        if (r.route) return r;
    }
    if (!h->f32_lane_node || h->small_mode == 6) return r;
    r.wp = plan_wave_f32(h, h->small_mode != -1, want_llr, batch);
    if (r.wp.waves) r.route = r.wp.team ? 4 : 3;
    return r;
}

int ldpc_hip_bp_f32_route(const ldpc_hip_bp *h, int64_t batch, int32_t want_llr, int32_t *route) {
    if (!h || !route) return fail(LDPC_HIP_ERR_INVALID, "null argument");
    if (batch < 0) return fail(LDPC_HIP_ERR_INVALID, "negative batch");
    *route = plan_f32_route(h, batch, want_llr != 0).route;
    return LDPC_HIP_OK;
}

// The float32 message mode's on-chip routes, called by decode_f32 (host_f32.h) after its refusals: plan_f32_route.  *took = false: no on-chip kernel
// takes the batch -- decode_f32 goes on with its per-pass kernels.
int decode_onchip_f32(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took) {
    const DecodeIo io = {synd, batch, decoding, llr, iters, conv};
    const OnchipRoute r = plan_f32_route(h, batch, llr != nullptr);
    *took = r.route != 0;
    if (r.route == 1 || r.route == 2) return decode_edge_f32(h, r.ep, io);
    if (r.route >= 3) return decode_wave_f32(h, r.wp, io);
    return LDPC_HIP_OK;
}

// ---- row priors on the lane = node kernel (bp_wave_rp_kernel.h; instantiated in tu_onchip_wave_rp.hip): min-sum on the codes beyond both lane = edge ladders ----
// The plan is plan_wave_lds's with this kernel's sizes: the relay kernel's shared tables, bp_wave_kernel's private region with the posterior copy (the
// kernel has no llr_direct form).  (solo_cap 16: the instantiations' 76 .. 137 VGPRs allow 16 wavefronts per compute unit, 12 where compiled for 12)
static WavePlan plan_wave_rp(const ldpc_hip_bp *h, bool forced, int64_t batch) {
    static const WaveLdsKernel k = {wave_rp_lds_shared, [](int mp, int np, int dr) { return wave_rp_lds_private(mp, np, dr); }, nullptr, wave_ms_waves, 16};
    return plan_wave_lds(h, forced, batch, k, -1, WAVE_RP_LDS_STATIC);
}

// h->row_probs [batch][n] -> out [batch][np + 2], every row padded as wave_prior_pad_kernel pads the shared priors: the log-ratio of column j < n by the
// IEEE division and the bit-exact log twin of row_priors_rowmajor_kernel (io_kernels.h), 1.0 for the columns n .. np - 1, DBL_MAX at np, 1.0 at np + 1.
// A thread reads probs only where j < n: row b's padding never looks at row b + 1 or past the array's end.
__global__ void __launch_bounds__(256) wave_rp_prior_kernel(const double *__restrict__ probs, int64_t batch, int n, int np, double *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) double log_tab[256];
    log_tab[threadIdx.x] = ldpc_math::k_log_tab[threadIdx.x];
    __syncthreads();
    const int64_t stride = np + 2, items = batch * stride;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / stride;
        const int j = (int)(t - b * stride);
        double v = j == np ? DBL_MAX : 1.0;
        if (j < n) {
            const double p = probs[b * (int64_t)n + j];
            v = ldpc_math::log_libm((1.0 - p) / p, log_tab);
        }
        out[t] = v;
    }
}

// The padded layout, not the unpadded one: the kernel then indexes a syndrome's row exactly as bp_wave_kernel indexes prior_g --
// phantom entries and padding columns need no select in the bit pass -- for (np + 2) / n of the bytes.  The table lives in rowp_llr, the row-prior
// decodes' grow-only buffer, whole batch; the handle's own priors (d_llr0, w_prior) are neither read nor written.
static int decode_wave_rp(ldpc_hip_bp *h, const WavePlan &p, const DecodeIo &io) {
    const WaveRpKernel kern = wave_rp_kernel(p.dr, p.dc, p.team);
    if (!kern) return fail(LDPC_HIP_ERR_UNSUPPORTED, "row priors: no lane = node kernel was built for rows of %d, columns of %d", p.dr, p.dc);
    int rc;
    WaveRpArgs ra = {};
    if ((rc = ensure_wave_tables(h, p)) || (rc = wave_counters(h, wave_static_teams(p, io.batch)))) return rc;  // (no OSD hook: bposd_device arms none for row priors)
    const size_t items = (size_t)io.batch * (size_t)(p.np + 2);
    if ((rc = h->rowp_llr.ensure(sizeof(double) * items))) return rc;
    LDPC_LAUNCH(wave_rp_prior_kernel, flat_grid(items), dim3(256), 0, h->stream, h->row_probs, io.batch, h->n, p.np, (double *)h->rowp_llr.p);
    HIPCHK(hipGetLastError());
    ra.rowp = (const double *)h->rowp_llr.p;
    return launch_wave(h, p, kern, ra, ra.w, io);
}

// Row priors on the lane = node kernel under the default modes (-1, 1, 6)?  Debug switch WAVE_RP: 0 off, 1 on, unset: the default below -- the route, by
// the rule fixed before it was measured: on one MI355X in one job, B = 65 536, min-sum 30, it beat the better of the parent's two
// row-prior runs 4.71x on HGP [[400,16]] (44.7 against 9.50 M syndromes/s, the slot kernel), 11.9x on the [[1600,64]] hypergraph product (9.77 against
// 0.823 M/s, per-pass) and 4.73x on BB144 x 12 rounds (14.0 against 2.97 M/s, per-pass), run-to-run spreads <= 3.4 % (profiles/row_priors_wave.jsonl).
// Modes 3, 4 and 5 take the kernel whatever this says.
static constexpr bool k_wave_rp_default = true;
static bool wave_rp_route(const ldpc_hip_bp *h) {
    if (h->small_mode >= 3 && h->small_mode <= 5) return true;
    const int s = h->sw("WAVE_RP");
    return s >= 0 ? s != 0 : k_wave_rp_default;
}

// Which route a row-prior decode of `batch` syndromes takes -- one decision for decode_onchip and ldpc_hip_bp_row_prior_route: 0 the per-pass
// kernels, 1 bp_edge_rp, 2 bp_edge8_rp, 3 / 4 bp_wave_rp with one wavefront / a team per syndrome, 5 the slot kernel (bp_small_kernel<., ., RP>).
// The order is decode_onchip's own, and `took` means what it means there -- an on-chip kernel takes the PLAIN decode of this code:
//   1. min-sum on a code plan_edge or plan_edge8 takes (modes -1, 1, 6): their row-prior forms where edge_rp_route says so;
//   2. min-sum on a code no earlier branch took -- neither bp_wave_ps (product-sum) nor a lane = edge family -- and plan_wave_rp takes (any mode
//      but 0 and 2): bp_wave_rp_kernel where wave_rp_route says so; a code an earlier branch took stays where it went before this route;
//   3. the slot kernel, with as many slots (<= 4) as fit the budget: 150 KiB where the mode forces it or another on-chip kernel takes the code's
//      plain decode, 39.5 KiB otherwise;
//   4. the per-pass kernels, if not even one slot fits -- and for everything under mode 0.
struct RowPriorRoute { int route = 0; EdgePlan ep; WavePlan wp; int slots = 0; };
static RowPriorRoute plan_row_prior_route(const ldpc_hip_bp *h, int64_t batch, bool want_llr) {
    RowPriorRoute r;
    const int mode = h->small_mode;
    if (!(mode != 0 && onchip_bound(h, batch))) return r;
    bool took = false;
    if (mode < 2 || mode == 6) took = plan_wave_ps(h, mode == 1, want_llr, batch).waves != 0;
    if (!took && (mode == -1 || mode == 1 || mode == 6)) {
        r.ep = plan_edge_family(h);
        if (r.ep.family) {
            took = true;
            if (edge_rp_route(h)) { r.route = r.ep.family; return r; }
        }
    }
    if (!took && mode != 2) {
        const bool forced = mode == 1 || (mode >= 3 && mode != 6);
        if (h->bp_method == LDPC_HIP_MINIMUM_SUM && wave_rp_route(h)) {
            r.wp = plan_wave_rp(h, forced, batch);
            if (r.wp.waves) { r.route = r.wp.team ? 4 : 3; return r; }
        }
        took = plan_wave(h, forced, want_llr, batch).waves != 0;
    }
    const size_t budget = (mode == 1 || mode == 2 || took) ? 150u * 1024u : 39u * 1024u + 512u;
    for (int sl = 4; sl >= 1 && !r.slots; --sl)
        if (small_lds_bytes(h, sl, true) <= budget) r.slots = sl;
    if (r.slots) r.route = 5;
    return r;
}

int row_prior_route(const ldpc_hip_bp *h, int64_t batch, bool want_llr) { return plan_row_prior_route(h, batch, want_llr).route; }

// Which on-chip kernel (if any) takes this batch: called by decode_device (host_stream.h) before it falls back to the streamed tiles.
// Row priors (h->row_probs): plan_row_prior_route above says which kernels decode them -- the row-prior forms of the lane = edge families, of the
// lane = node kernel, the SLOT kernel, which reads every syndrome's own priors too (bp_small_kernel<., ., RP>), or the per-pass kernels (took = false).
int decode_onchip(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took) {
    *took = false;
    const DecodeIo io = {synd, batch, decoding, llr, iters, conv};
    const bool rp = h->row_probs != nullptr;
    if (h->variant == Variant::Memory) {
        // Memory min-sum (ldpc_hip_bp_set_memory), by plan_relay_route: a code that plan_edge or plan_edge8 takes runs on their memory forms, a code
        // plan_wave_relay takes on bp_wave_relay_kernel as ONE relay leg of max_iter iterations that stops at its first solution -- that decode's bits;
        // every other code -- and every code under mode 0 -- goes to the per-pass memory kernels (took = false).  The persistent ring kernel,
        // bp_wave_kernel, the slot kernel and the resident workgroup know nothing of the memory and never see such a decode.
        const OnchipRoute r = plan_relay_route(h, batch);
        *took = r.route != 0;
        if (r.route == 1 || r.route == 2) return decode_edge_mem(h, r.ep, io);
        if (r.route >= 3) return decode_wave_relay(h, r.wp, (const double *)h->mem_ag.p, 1, nullptr, 1, io);
        return LDPC_HIP_OK;
    }
    if (rp) {  // every syndrome its own priors: one decision, the one ldpc_hip_bp_row_prior_route reports
        const RowPriorRoute r = plan_row_prior_route(h, batch, llr != nullptr);
        *took = r.route != 0;
        if (r.route == 1 || r.route == 2) return decode_edge_rp(h, r.ep, io);
        if (r.route == 3 || r.route == 4) return decode_wave_rp(h, r.wp, io);
        if (r.route == 5) return decode_small(h, synd, batch, decoding, llr, iters, conv, r.slots);
        return LDPC_HIP_OK;
    }
    if (h->small_mode != 0 && onchip_bound(h, batch)) {
        // small code: keep the messages on chip.  Bounded degrees: one wavefront per syndrome (bp_wave_kernel).
        // Otherwise the slot kernel -- auto: the most resident syndromes (<= 4) per workgroup that still leave
        // four workgroups per CU (<= 39.5 KiB each); forced: whatever fits in 150 KiB
        if (h->small_mode < 2 || h->small_mode == 6) {  // (mode 6: as -1 wherever the lane = edge variants do not apply) product-sum: one lane per entry keeps the lanes busy with transcendentals
            const WavePsPlan pp = plan_wave_ps(h, h->small_mode == 1, llr != nullptr, batch);
            if (pp.waves) { *took = true; return decode_wave_ps(h, pp, io); }
        }
        if (h->small_mode == -1 || h->small_mode == 1 || h->small_mode == 6) {  // min-sum on the surface-code family: lane = edge
            const EdgePlan ep = plan_edge_family(h);
            if (ep.family) { *took = true; return decode_edge(h, ep, io); }
        }
        if (h->small_mode != 2) {
            const WavePlan wp = plan_wave(h, h->small_mode == 1 || (h->small_mode >= 3 && h->small_mode != 6), llr != nullptr, batch);
            if (wp.waves) { *took = true; return decode_wave(h, wp, io); }
        }
        int slots = 0;
        const size_t budget = (h->small_mode == 1 || h->small_mode == 2) ? 150u * 1024u : 39u * 1024u + 512u;
        for (int sl = 4; sl >= 1 && !slots; --sl)
            if (small_lds_bytes(h, sl) <= budget) slots = sl;
        if (slots) { *took = true; return decode_small(h, synd, batch, decoding, llr, iters, conv, slots); }
    }
    return LDPC_HIP_OK;
}

// ---- a single decode() through the resident workgroup ------------------------------------------------------------------------------------
// What the reference's callers do is `for shot: decoder.decode(shot)`: one syndrome per call, host arrays.  A launch and its completion
// cost ~15 us of such a call and the kernel's table set-up ~10 us more (profiles/r4_single_decode_latency.txt) -- so the workgroup that
// decoded one syndrome STAYS (bp_wave_ps_kernel<., ., ., TEAM>, WavePsArgs::mail): the next call writes its syndrome into the handle's
// host-mapped block, bumps the request word, and spins on the served word; the workgroup polls the request word over PCIe, decodes with
// the tables it already has in LDS, writes the results into the block and bumps the served word.  It leaves after `linger` (100 us)
// without a request -- it cannot outlive a caller by more than that, and a torch.cuda.synchronize() behind a
// decode() waits that long at most -- or at once when told to (resident_retire: parameters or priors changed, handle destroyed).
// The block's layout for one syndrome is decode_batch_staged's (host_decode_abi.h); the syndrome is already in it.
void resident_retire(ldpc_hip_bp *h) {
    auto &r = h->res;
    if (!h->pin_host || !r.stream) return;
    volatile unsigned *mail = reinterpret_cast<volatile unsigned *>(h->pin_host + ldpc_hip_bp::PIN_MAIL);
    if (r.launched) {
        __atomic_store_n(const_cast<unsigned *>(mail + 3), 1u, __ATOMIC_SEQ_CST);
        (void)hipStreamSynchronize(r.stream);
        __atomic_store_n(const_cast<unsigned *>(mail + 3), 0u, __ATOMIC_SEQ_CST);
        r.launched = false;
    }
}

int decode_onchip_resident(ldpc_hip_bp *h, bool want_llr, bool *took) {
    *took = false;
    (void)want_llr;
    // (the same predicate as decode_onchip's bp_wave_ps branch: a caller who FORCED another small-code kernel -- modes 3, 4, 5, 2 -- gets that kernel)
    if (h->sw("RESIDENT") == 0 || !h->pin_host || h->schedule != 1 || !(h->small_mode < 2 || h->small_mode == 6) || h->small_mode == 0) return LDPC_HIP_OK;
    if (!onchip_bound(h, 1)) return LDPC_HIP_OK;
    const WavePsPlan p = plan_wave_ps(h, h->small_mode == 1, true, 1);  // (the posteriors are always formed: one plan whatever the caller asks for)
    if (!p.waves || !p.team) return LDPC_HIP_OK;
    auto &r = h->res;
    int rc;
    if (!r.stream) {
        if (hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&r.ended, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (r.stream) { (void)hipStreamDestroy(r.stream); r.stream = nullptr; }
            return LDPC_HIP_OK;
        }
    }
    unsigned *mail = reinterpret_cast<unsigned *>(h->pin_host + ldpc_hip_bp::PIN_MAIL);
    unsigned long long alpha_bits;
    std::memcpy(&alpha_bits, &h->ms_scaling_factor, 8);
    const unsigned long long key[6] = {((unsigned long long)(unsigned)h->max_iter << 32) | (unsigned)h->math_mode, h->priors_version, alpha_bits,
                                       ((unsigned long long)(unsigned)p.dr << 48) | ((unsigned long long)(unsigned)p.dc << 32) | (unsigned)p.waves,
                                       (unsigned long long)(uintptr_t)h->d_llr0, (unsigned long long)(unsigned)h->small_mode};
    if (r.launched && std::memcmp(key, r.key, sizeof key) != 0) resident_retire(h);  // (launched for other parameters: it leaves, a new one comes)
    const size_t m = (size_t)h->m, n = (size_t)h->n;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_dec = up16(m), o_llr = o_dec + up16(n), o_it = o_llr + up16(n * 8), o_cv = o_it + up16(4);
    auto launch = [&]() -> int {
        if ((rc = ensure_wave_ps_tables(h, p))) return rc;
        WavePsArgs a = {};
        a.m = h->m; a.n = h->n; a.np = p.np; a.max_iter = h->max_iter;
        a.batch = 1;
        wave_table_fields(h, p, a);
        a.llr0 = h->d_llr0;
        unsigned char *dv = h->pin_dev;
        a.synd = dv; a.decoding = dv + o_dec; a.llr = (double *)(dv + o_llr); a.iters = (int32_t *)(dv + o_it); a.conv = dv + o_cv;
        a.next = nullptr;
        a.clk = nullptr;
        a.lds_shared = (int32_t)p.shared; a.lds_per_wave = (int32_t)p.per_wave;
        a.mail = reinterpret_cast<unsigned *>(h->pin_dev + ldpc_hip_bp::PIN_MAIL);
        a.served0 = __atomic_load_n(mail + 1, __ATOMIC_ACQUIRE);
        const int linger_us = 100;
        a.linger_ticks = (unsigned)linger_us * 100u;  // (the constant-rate counter runs at 100 MHz)
        const size_t dyn = p.shared + p.per_wave;
        if (dyn > 48u * 1024u) HIPCHK(hipFuncSetAttribute((const void *)p.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        __atomic_store_n(mail + 3, 0u, __ATOMIC_SEQ_CST);
        __atomic_store_n(mail + 2, 1u, __ATOMIC_SEQ_CST);
        LDPC_LAUNCH(p.kern, dim3(1), dim3((unsigned)(p.waves * 64)), (unsigned)dyn, r.stream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(r.ended, r.stream));
        std::memcpy(r.key, key, sizeof key);
        r.launched = true;
        return LDPC_HIP_OK;
    };
    if (r.launched && __atomic_load_n(mail + 2, __ATOMIC_ACQUIRE) == 0u) {  // it said it was leaving: see it gone before the next one is launched
        HIPCHK(hipStreamSynchronize(r.stream));
        r.launched = false;
    }
    if (!r.launched) {
        if (r.seq == 0) { __atomic_store_n(mail + 0, 0u, __ATOMIC_SEQ_CST); __atomic_store_n(mail + 1, 0u, __ATOMIC_SEQ_CST); }
        if ((rc = launch())) return rc;
    }
    const unsigned seq = ++r.seq ? r.seq : ++r.seq;  // (never 0: the words' initial value)
    __atomic_store_n(mail + 0, seq, __ATOMIC_SEQ_CST);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(mail + 1, __ATOMIC_ACQUIRE) == seq) break;
        if (__atomic_load_n(mail + 2, __ATOMIC_SEQ_CST) == 0u) {
            // it is leaving (or gone): either it saw this request on its last look and serves it before it goes, or it did not
            const hipError_t q = hipEventQuery(r.ended);
            if (q == hipSuccess) {
                r.launched = false;
                if (__atomic_load_n(mail + 1, __ATOMIC_ACQUIRE) == seq) break;
                if ((rc = launch())) return rc;  // (the new one finds the request waiting)
            } else if (q != hipErrorNotReady) {
                return fail(LDPC_HIP_ERR_DEVICE, "the resident decode kernel failed: %s", hipGetErrorString(q));
            } else {
                (void)hipGetLastError();
            }
        }
        if ((spins & 0xfffu) == 0xfffu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
            // The resident workgroup was never scheduled (the GPU is busy with someone else's long kernel) or is stuck: tell it to leave, wait
            // for its stream, and if it did serve the request on its way out take that; otherwise withdraw the request (the next resident
            // kernel starts from served = request: no stale sequence number) and let the ordinary launch path decode this call.
            resident_retire(h);
            if (__atomic_load_n(mail + 1, __ATOMIC_ACQUIRE) == seq) break;
            __atomic_store_n(mail + 0, 0u, __ATOMIC_SEQ_CST);
            __atomic_store_n(mail + 1, 0u, __ATOMIC_SEQ_CST);
            r.seq = 0;
            return LDPC_HIP_OK;  // (*took stays false)
        }
        if ((spins & 0x3ffu) == 0x3ffu) std::this_thread::yield();  // (a core shared with the caller's other threads is not held hostage)
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    h->timed = false;
    h->accumulated_ms = 0.f;
    *took = true;
    return LDPC_HIP_OK;
}
