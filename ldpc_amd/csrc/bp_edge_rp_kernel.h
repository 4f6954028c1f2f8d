// bp_edge_rp_kernel.h -- bp_edge_rp_kernel, bp_edge8_rp_kernel: the lane = edge min-sum kernels with ROW PRIORS (every syndrome its own priors)
// Part of libldpc_hip.so: instantiated in tu_onchip_rp.hip, launched by host_onchip.h (decode_edge_rp, decode_edge8_rp).
#pragma once

#include "bp_edge_kernel.h"

// ldpc_hip_*_decode_batch_priors on a code of the lane = edge families (bp_edge_kernel.h): the general forms of bp_edge_kernel and
// bp_edge8_kernel (UNIFORM = false, NOCLAMP = false -- the clamp to DBL_MAX stays), restated operation by operation, with ONE difference:
// the prior registers prv[r] are not filled once per kernel from EdgeArgs::prior_s but inside the syndrome loop, for the syndrome b the
// wavefront holds, from row b of `rowp` [batch][n] -- the log-ratios log((1 - P[b][j]) / P[b][j]) (io_kernels.h: row_priors_rowmajor_kernel,
// the operations of upload_priors) -- at the slot's column.  Row-major because a lane is an edge: the R loads of a wavefront for one
// syndrome touch the 8 n contiguous bytes of its row.  The slot's column is RE-READ per syndrome from the slot table (EdgeArgs::scol, 256 R
// bytes that stay in cache) rather than kept in R more registers: with it in registers bp_edge_rp_kernel<13 .. 16> and
// bp_edge8_rp_kernel<10, 3>, <12, 3>, <9, 4> spill (up to 32 VGPRs, 132 bytes of scratch a lane), and the two dependent loads a syndrome
// cost about a microsecond of the tens a wavefront spends on one.  A phantom lane is known by its partner address (the +inf slot) and gets
// the prior +inf, as in prior_s.
// The `0.0 + x` / `x + 0.0` argument of bp_edge_kernel.h holds as it does there: a row prior is log((1 - p) / p) by the same division and
// the same log as the handle's, never -0.0 (p = 0.5 gives log(1.0) = +0.0), and a sum is -0.0 only if both terms are.
// Nothing here reads EdgeArgs::prior_s / prior_u (the handle's e_prior stays as the last plain call left it).  Results are bit-identical to
// the slot kernel's (bp_small_kernel<., ., true>) and to the reference's update_channel_probs + decode loop (tests/test_gpu_row_priors_edge.py).
struct EdgeRpArgs {
    EdgeArgs e;           // prior_s, prior_u: not read
    const double *rowp;   // [batch][n] log-ratio of every syndrome's own channel probabilities
};
struct Edge8RpArgs {
    Edge8Args e;          // prior_s, prior_u: not read
    const double *rowp;
};

typedef void (*EdgeRpKernel)(const EdgeRpArgs);
typedef void (*Edge8RpKernel)(const Edge8RpArgs);
// The instantiations live in tu_onchip_rp.hip; the host side (host_onchip.h, in tu_onchip.hip) asks for them by the plan's numbers.
// nullptr: no such instantiation (the ladders are those of plan_edge and plan_edge8).
EdgeRpKernel edge_rp_kernel(int rounds);
Edge8RpKernel edge8_rp_kernel(int rounds, int dc);

template <int R>
__global__ void __launch_bounds__(64, 4) bp_edge_rp_kernel(const EdgeRpArgs ra) {
    using namespace edge_detail;
    const EdgeArgs &a = ra.e;
    typedef EdgeRpArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_lds[];
    lds_f64 *X = (lds_f64 *)edge_lds;  // [R * 64] check_to_bit of every slot, [R * 64] = +0.0 for good
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr uint64_t LOW = 0x1111111111111111ull;

    // per lane and round, for the whole kernel: partner address; per round: which lanes are first entries.  prv[r]: per SYNDROME
    double prv[R], msg[R];
    int paddr[R];
    uint64_t k0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
        paddr[r] = (int)a.partner[s];
        k0[r] = __ballot(a.kind[s] == 1);
    }
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_VARIANT_ARG(static_per), b1 = b0 + LDPC_EDGE_VARIANT_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        // THIS syndrome's priors (b is wave-uniform: whichever row the wavefront pulled, never its slot's or its predecessor's)
        const auto pb = global_ptr(LDPC_KERNARG(ARGS_T, rowp)) + (int64_t)b * n;
        const auto scol_t = global_ptr(LDPC_EDGE_VARIANT_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = paddr[r] == ZERO + 1 ? __builtin_inf() : pb[scol_t[r * 64 + lane]];  // phantom lanes: +inf (bp_edge_kernel.h); theirs is column 0 in the table
        uint64_t sy[R];
        bool never = false;
        const auto sb = global_ptr(LDPC_EDGE_VARIANT_ARG(synd)) + (int64_t)b * m;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r * 16 + (lane >> 2);
            const int byte = row < m ? (int)sb[row] : 0;
            sy[r] = __ballot((byte & 1) != 0) & LOW;
            never = never || __ballot(byte > 1) != 0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = prv[r];  // initialise_log_domain_bp (bp.hpp:147-157)

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
            // ---- check pass: msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot ----
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0);
                const double x1 = quad_perm<0xB1>(cur);               // lane ^ 1
                const double pairmin = min_abs(cur, x1);
                const double other = quad_perm<0x4E>(pairmin);        // the other pair's minimum (lane ^ 2)
                const double mag = fmin_pos(min_abs(x1, other), dbl_max);  // over the three other entries, from DBL_MAX down
                int shi;  // high word of +-alpha: sign = row parity (syndrome included) + own
                if (r < EDGE_V1) {
                    const uint64_t par = nibble_parity_low(neg ^ sy[r]);
                    const int own = select_by_mask(al.hi, al.nhi, neg);
                    const int rowbit = select_by_mask(0, (int)0x80000000, par);
                    shi = own ^ __builtin_amdgcn_mov_dpp(rowbit, 0x00, 0xf, 0xf, true);  // quad_perm [0, 0, 0, 0]
                } else {
                    const uint64_t flip = spread_nibble(nibble_parity_low(neg ^ sy[r])) ^ neg;
                    shi = select_by_mask(al.hi, al.nhi, flip);
                }
                const double c = mag * __hiloint2double(shi, al.lo);
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
            // ---- bit pass: the partner's message; log-ratio, decision, new bit_to_check ----
            uint64_t bad = 0;
#pragma unroll
            for (int r0 = 0; r0 < R; r0 += EDGE_G) {
                double cpv[EDGE_G];
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g)
                    if (r0 + g < R) cpv[g] = X[paddr[r0 + g]];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < EDGE_G; ++g) {
                    const int r = r0 + g;
                    if (r >= R) break;
                    const double cp = cpv[g];
                    const double c = msg[r];
                    const double b2c = prv[r] + cp;
                    const double l1 = b2c + c;             // second entry of its column: (prior + c0) + c1 with c0 = the partner's
                    const double l0 = (prv[r] + c) + cp;   // first entry: c0 = its own
                    uint64_t d;
                    if (r < EDGE_V2) {
                        const double l = __hiloint2double(select_by_mask(__double2hiint(l1), __double2hiint(l0), k0[r]),
                                                          select_by_mask(__double2loint(l1), __double2loint(l0), k0[r]));
                        d = __ballot(l <= 0.0);
                    } else {
                        const uint64_t d1 = __ballot(l1 <= 0.0);
                        d = d1 ^ ((__ballot(l0 <= 0.0) ^ d1) & k0[r]);  // (phantom lanes: neither)
                    }
                    bad |= nibble_parity_low(d) ^ sy[r];  // candidate syndrome vs syndrome (bp.hpp:292-302), bit 0 of every nibble
                    msg[r] = b2c;
                }
            }
            unsat = never || (bad & LOW) != 0;
        } while (unsat && it < a.max_iter);

        // ---- outputs (as bp_edge_kernel): the first entry of a column parks the column's log-ratio at X[column], whole rows leave ----
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = (prv[r] + X[r * 64 + lane]) + X[paddr[r]];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = scol_t[r * 64 + lane];
            if ((k0[r] >> lane) & 1ull) X[j] = msg[r];
        }
        {
            const auto dp = global_ptr(LDPC_EDGE_VARIANT_ARG(decoding)) + (int64_t)b * n;
            auto lp = global_ptr(LDPC_EDGE_VARIANT_ARG(llr));
            if (lp) lp += (int64_t)b * n;
            for (int j = lane; j < n; j += 64) {
                const double l0 = X[j];
                dp[j] = l0 <= 0.0 ? 1 : 0;
                if (lp) lp[j] = l0;
            }
        }
        {
            const auto ip = global_ptr(LDPC_EDGE_VARIANT_ARG(iters));
            const auto cp = global_ptr(LDPC_EDGE_VARIANT_ARG(conv));
            if (lane == 0) {
                if (ip) ip[b] = it;
                if (cp) cp[b] = unsat ? 0 : 1;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (see bp_edge_kernel: the wavefront is whole before lane 0 pulls the next syndrome)
      }
        if (!work_pool_next(LDPC_EDGE_VARIANT_ARG(next), LDPC_EDGE_VARIANT_ARG(dyn_base), LDPC_EDGE_VARIANT_ARG(pool_per), LDPC_EDGE_VARIANT_ARG(chunk), (int)LDPC_EDGE_VARIANT_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_VARIANT_ARG(clk), clk_stamp);
}

template <int R, int DC>
__global__ void __launch_bounds__(64, 4) bp_edge8_rp_kernel(const Edge8RpArgs ra) {
    using namespace edge_detail;
    const Edge8Args &a = ra.e;
    typedef Edge8RpArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    static_assert(DC >= 2 && DC <= 4, "columns of 2 .. 4 entries");
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_lds[];
    lds_f64 *X = (lds_f64 *)edge_lds;
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr uint64_t LOW = 0x0101010101010101ull;

    double prv[R], msg[R];
    int caddr[R][DC];
    uint64_t kmask[R][DC - 1];  // lanes whose entry is the (j + 1)-th of its column, j < DC - 1
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
#pragma unroll
        for (int j = 0; j < DC; ++j) caddr[r][j] = (int)a.cpos[(size_t)j * (R * 64) + s];
        const int kd = a.kind[s];
#pragma unroll
        for (int j = 0; j < DC - 1; ++j) kmask[r][j] = __ballot(kd == j + 2);
    }
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    int b0 = (int)blockIdx.x * LDPC_EDGE_VARIANT_ARG(static_per), b1 = b0 + LDPC_EDGE_VARIANT_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        // THIS syndrome's priors (see bp_edge_rp_kernel)
        const auto pb = global_ptr(LDPC_KERNARG(ARGS_T, rowp)) + (int64_t)b * n;
        const auto scol_t = global_ptr(LDPC_EDGE_VARIANT_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = caddr[r][0] == ZERO + 1 ? __builtin_inf() : pb[scol_t[r * 64 + lane]];  // phantom lanes (theirs is the dummy slot in the table): +inf
        uint64_t sy[R];
        bool never = false;
        const auto sb = global_ptr(LDPC_EDGE_VARIANT_ARG(synd)) + (int64_t)b * m;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = r * 8 + (lane >> 3);
            const int byte = row < m ? (int)sb[row] : 0;
            sy[r] = __ballot((byte & 1) != 0) & LOW;
            never = never || __ballot(byte > 1) != 0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = prv[r];  // initialise_log_domain_bp (bp.hpp:147-157); phantom lanes: +inf

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
            // ---- check pass (bp.hpp:220-273): minimum over the seven other lanes of the group, sign by the group's parity ----
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0);
                const double x1 = quad_perm<0xB1>(cur);                // lane ^ 1
                const double pairmin = min_abs(cur, x1);
                const double otherpair = quad_perm<0x4E>(pairmin);     // lane ^ 2: the other pair of the quad
                const double inquad = min_abs(x1, otherpair);          // the three others of the quad
                const double quadmin = min_abs(pairmin, otherpair);    // ... and the whole quad, for the other quad
                const double otherquad = xor4(quadmin);
                const double mag = fmin_pos(min_abs(inquad, otherquad), dbl_max);  // the seven other entries, from DBL_MAX down
                const uint64_t flip = spread_byte(byte_parity_low(neg ^ sy[r])) ^ neg;
                const double c = mag * __hiloint2double(select_by_mask(al.hi, al.nhi, flip), al.lo);
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
            // ---- bit pass (bp.hpp:276-318): the column's entries in order; log-ratio, decision, the lane's own bit_to_check ----
            uint64_t bad = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double c[DC];
#pragma unroll
                for (int j = 0; j < DC; ++j) c[j] = X[caddr[r][j]];
                const double pr = prv[r];
                double pre[DC];  // pre[k] = prior + c0 + ... + c_{k-1}
                double t = pr;
#pragma unroll
                for (int j = 0; j < DC; ++j) { pre[j] = t; t += c[j]; }
                const uint64_t d = __ballot(t <= 0.0);  // (phantom lanes: +inf or NaN, never <= 0)
                bad |= byte_parity_low(d) ^ sy[r];
                double cand[DC];
                double sfx = c[DC - 1];
                cand[DC - 1] = pre[DC - 1];
                cand[DC - 2] = pre[DC - 2] + sfx;
#pragma unroll
                for (int k = DC - 3; k >= 0; --k) { sfx += c[k + 1]; cand[k] = pre[k] + sfx; }
                double b2c = cand[0];
#pragma unroll
                for (int k = 1; k < DC; ++k) b2c = select_f64(b2c, cand[k], kmask[r][k - 1]);
                msg[r] = b2c;
            }
            unsat = never || (bad & LOW) != 0;
        } while (unsat && it < a.max_iter);

        // ---- outputs: as bp_edge8_kernel (phantom lanes park theirs at the dummy slot behind +inf) ----
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double t = prv[r];
#pragma unroll
            for (int j = 0; j < DC; ++j) t += X[caddr[r][j]];
            msg[r] = t;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = msg[r];
        {
            const auto dp = global_ptr(LDPC_EDGE_VARIANT_ARG(decoding)) + (int64_t)b * n;
            auto lp = global_ptr(LDPC_EDGE_VARIANT_ARG(llr));
            if (lp) lp += (int64_t)b * n;
            for (int j = lane; j < n; j += 64) {
                const double t = X[j];
                dp[j] = t <= 0.0 ? 1 : 0;
                if (lp) lp[j] = t;
            }
        }
        {
            const auto ip = global_ptr(LDPC_EDGE_VARIANT_ARG(iters));
            const auto cp = global_ptr(LDPC_EDGE_VARIANT_ARG(conv));
            if (lane == 0) {
                if (ip) ip[b] = it;
                if (cp) cp[b] = unsat ? 0 : 1;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (see bp_edge_kernel)
      }
        if (!work_pool_next(LDPC_EDGE_VARIANT_ARG(next), LDPC_EDGE_VARIANT_ARG(dyn_base), LDPC_EDGE_VARIANT_ARG(pool_per), LDPC_EDGE_VARIANT_ARG(chunk), (int)LDPC_EDGE_VARIANT_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_VARIANT_ARG(clk), clk_stamp);
}
