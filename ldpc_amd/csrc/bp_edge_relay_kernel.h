// bp_edge_relay_kernel.h -- bp_edge_relay_kernel, bp_edge8_relay_kernel: Relay-BP on the lane = edge min-sum kernels, all legs of a syndrome in one launch
// Part of libldpc_hip.so: instantiated in tu_onchip_relay.hip, launched by host_onchip.h (decode_edge_relay, decode_edge8_relay).
#pragma once

#include "bp_edge_mem_kernel.h"
#include "relay_common.h"

// ldpc_hip_bp_set_relay on a code of the lane = edge families: the check and bit passes of bp_edge_mem_kernel / bp_edge8_mem_kernel
// (bp_edge_mem_kernel.h), operation by operation, inside a loop over the legs -- one wavefront per syndrome, M in the registers prv[r], nothing
// leaves the chip between legs.  Per leg: a and gamma of the lane's slots come from the leg's slot tables (EdgeRelayArgs::ag_s, [legs][2][R * 64];
// edge_relay_table_kernel, host_onchip.h) -- up to KEEP rounds into registers for the leg, above re-read in every bit pass as the memory kernels
// do; the iteration count starts again at 1 (the scaling factor 0 counts the leg's iterations) and runs to leg_iters[leg].  Leg 0 starts as the
// memory decode: messages and M = L0.  A later leg keeps prv[r] -- M, the posterior of the previous leg's last bit pass -- and forms its initial
// messages from it: msg[r] = gamma == 0 ? a : a + gamma * prv[r] (a IS L0 where gamma == 0; a phantom lane: +inf).
// A leg that ends with the syndrome reproduced is a solution: the posteriors are parked at X[column] as the output pass does -- over the
// check-to-bit slots, which the next leg's first check pass rewrites in full before any bit pass reads one -- the weight is formed from them
// (relay_weight: lanes stride the columns, a butterfly over the wavefront), and if it is strictly smaller than the best so far the row's decoding
// and llr go to global memory, over an earlier solution's.  stop_after solutions end the row.  A row without any solution writes the last leg's
// last bit pass.  iters = the iterations of all legs run, conv = a solution was found.
// Results are bit-identical to the per-pass leg loop (host_stream.h: decode_relay) and to the NumPy restatement (tests/relay_bp_util.py).
struct EdgeRelayArgs {
    EdgeArgs e;                 // prior_s: L0 per slot (leg 0's messages and M); max_iter, prior_u: not read
    const double *ag_s;         // [legs][2][R * 64]: a, then gamma, of every slot, per leg; phantom: +inf and 0
    const int32_t *leg_iters;   // [legs]
    const double *llr0;         // [n] L0 per column (the weight)
    int32_t legs, stop_after;
};
struct Edge8RelayArgs {
    Edge8Args e;
    const double *ag_s;
    const int32_t *leg_iters;
    const double *llr0;
    int32_t legs, stop_after;
};

typedef void (*EdgeRelayKernel)(const EdgeRelayArgs);
typedef void (*Edge8RelayKernel)(const Edge8RelayArgs);
// The instantiations live in tu_onchip_relay.hip; nullptr: no such instantiation (the ladders are those of plan_edge and plan_edge8).
EdgeRelayKernel edge_relay_kernel(int rounds);
Edge8RelayKernel edge8_relay_kernel(int rounds, int dc);

// Wavefronts per SIMD the instantiations are compiled for; the host sizes its grid by them (launch_edge_relay).  What each instantiation
// compiles to is listed in DESIGN.md section 7d: the leg loop costs a handful of registers over the memory twin, and the instantiations that
// would spill at the twin's launch bounds get one wavefront per SIMD fewer.
__host__ __device__ constexpr int edge_relay_waves(int rounds) { return rounds <= 12 ? 4 : 3; }
__host__ __device__ constexpr int edge8_relay_waves(int, int) { return 4; }

// What both kernels do with a leg's end (X, lane, n, b, unsat, last and the row's running best / nsol are the kernel's): see the header comment.
// PARK: the statement that parks prv[] at X[column].
#define LDPC_EDGE_RELAY_LEG_END(PARK)                                                                                     \
    if (!unsat || (last && nsol == 0)) {                                                                                  \
        PARK                                                                                                              \
        bool take = unsat;                                                                                                \
        if (!unsat) {                                                                                                     \
            const double w = relay_weight((const double *)LDPC_KERNARG(ARGS_T, llr0), n, lane, [&](int j) { return X[j] <= 0.0; }); \
            ++nsol;                                                                                                       \
            if (__ballot(w < best) != 0) { best = w; take = true; }  /* (every lane holds the same w: the ballot keeps the branch scalar) */ \
        }                                                                                                                 \
        if (take) {                                                                                                       \
            const auto dp = global_ptr(LDPC_EDGE_VARIANT_ARG(decoding)) + (int64_t)b * n;                                    \
            auto lp = global_ptr(LDPC_EDGE_VARIANT_ARG(llr));                                                                \
            if (lp) lp += (int64_t)b * n;                                                                                 \
            for (int j = lane; j < n; j += 64) {                                                                          \
                const double t = X[j];                                                                                    \
                dp[j] = t <= 0.0 ? 1 : 0;                                                                                 \
                if (lp) lp[j] = t;                                                                                        \
            }                                                                                                             \
        }                                                                                                                 \
    }

template <int R>
__global__ void __launch_bounds__(64, edge_relay_waves(R)) bp_edge_relay_kernel(const EdgeRelayArgs ma) {
    using namespace edge_detail;
    const EdgeArgs &a = ma.e;
    typedef EdgeRelayArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_lds[];
    lds_f64 *X = (lds_f64 *)edge_lds;  // [R * 64] check_to_bit of every slot, [R * 64] = +0.0 for good
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr uint64_t LOW = 0x1111111111111111ull;
    constexpr bool KEEP = R <= EDGE_MEM_KEEP;
    constexpr int G = EDGE_G;  // rounds per group of the bit pass

    // per lane and round, for the whole kernel: partner address; per round: which lanes are first entries.  (KEEP) a and gamma: per LEG.  prv[r]: per ITERATION
    double prv[R], msg[R], av[KEEP ? R : 1], gv[KEEP ? R : 1];
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
        {   // M = L0: leg 0's initial messages (initialise_log_domain_bp, bp.hpp:147-157), and what its first iteration's prior is formed from
            const auto l0_t = global_ptr(LDPC_EDGE_VARIANT_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // (phantom lanes: +inf)
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
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

        double best = __builtin_inf();
        int nsol = 0, total = 0;
        const int legs = LDPC_KERNARG(ARGS_T, legs), stop_after = LDPC_KERNARG(ARGS_T, stop_after);
        const auto scol_t = global_ptr(LDPC_EDGE_VARIANT_ARG(scol));
        for (int leg = 0; leg < legs; ++leg) {
            const gtab_t a_t = global_ptr(LDPC_KERNARG(ARGS_T, ag_s)) + (size_t)leg * (2 * R * 64);  // the leg's tables: a, then gamma
            const gtab_t g_t = a_t + R * 64;
            const int leg_iters = global_ptr(LDPC_KERNARG(ARGS_T, leg_iters))[leg];
            const bool last = leg == legs - 1;
            if (KEEP) {
#pragma unroll
                for (int r = 0; r < R; ++r) { av[KEEP ? r : 0] = a_t[r * 64 + lane]; gv[KEEP ? r : 0] = g_t[r * 64 + lane]; }
            }
            if (leg > 0) {  // the initial messages of a later leg, from M = prv[r] (phantom lanes: a = +inf by gamma = 0)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double as = KEEP ? av[KEEP ? r : 0] : a_t[r * 64 + lane], gs = KEEP ? gv[KEEP ? r : 0] : g_t[r * 64 + lane];
                    msg[r] = gs == 0.0 ? as : as + gs * prv[r];
                }
            }

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
                // ---- bit pass: the prior from M; the partner's message; log-ratio, decision, new bit_to_check; prv[r] <- the column's posterior ----
                uint64_t bad = 0;
#pragma unroll
                for (int r0 = 0; r0 < R; r0 += G) {
                    double cpv[G], asv[G], gsv[G];
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (r0 + g < R) {
                            cpv[g] = X[paddr[r0 + g]];
                            asv[g] = KEEP ? av[KEEP ? r0 + g : 0] : a_t[(r0 + g) * 64 + lane];  // (above KEEP rounds: beside the partner's message, a group at a time)
                            gsv[g] = KEEP ? gv[KEEP ? r0 + g : 0] : g_t[(r0 + g) * 64 + lane];
                        }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const int r = r0 + g;
                        if (r >= R) break;
                        const double cp = cpv[g];
                        const double c = msg[r];
                        const double pr = gsv[g] == 0.0 ? asv[g] : asv[g] + gsv[g] * prv[r];  // THIS iteration's prior, from M = prv[r]
                        const double b2c = pr + cp;
                        const double l1 = b2c + c;             // second entry of its column: (prior + c0) + c1 with c0 = the partner's
                        const double l0 = (pr + c) + cp;       // first entry: c0 = its own
                        // the column's posterior, the same value in both of its lanes
                        const double l = __hiloint2double(select_by_mask(__double2hiint(l1), __double2hiint(l0), k0[r]),
                                                          select_by_mask(__double2loint(l1), __double2loint(l0), k0[r]));
                        const uint64_t d = __ballot(l <= 0.0);  // (phantom lanes: +inf or NaN, never <= 0)
                        bad |= nibble_parity_low(d) ^ sy[r];  // candidate syndrome vs syndrome (bp.hpp:292-302), bit 0 of every nibble
                        msg[r] = b2c;
                        prv[r] = l;  // M of the next iteration, and of the next leg
                    }
                }
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < leg_iters);
            total += it;

            // ---- the leg's end: a solution, or the last leg of a row without one (the first entry of a column parks the column's log-ratio) ----
            LDPC_EDGE_RELAY_LEG_END(
                _Pragma("unroll") for (int r = 0; r < R; ++r) {
                    const int j = scol_t[r * 64 + lane];
                    if ((k0[r] >> lane) & 1ull) X[j] = prv[r];
                })
            if (nsol == stop_after) break;
        }
        {
            const auto ip = global_ptr(LDPC_EDGE_VARIANT_ARG(iters));
            const auto cp = global_ptr(LDPC_EDGE_VARIANT_ARG(conv));
            if (lane == 0) {
                if (ip) ip[b] = total;
                if (cp) cp[b] = nsol > 0 ? 1 : 0;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (see bp_edge_kernel: the wavefront is whole before lane 0 pulls the next syndrome)
      }
        if (!work_pool_next(LDPC_EDGE_VARIANT_ARG(next), LDPC_EDGE_VARIANT_ARG(dyn_base), LDPC_EDGE_VARIANT_ARG(pool_per), LDPC_EDGE_VARIANT_ARG(chunk), (int)LDPC_EDGE_VARIANT_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_VARIANT_ARG(clk), clk_stamp);
}

template <int R, int DC>
__global__ void __launch_bounds__(64, edge8_relay_waves(R, DC)) bp_edge8_relay_kernel(const Edge8RelayArgs ma) {
    using namespace edge_detail;
    const Edge8Args &a = ma.e;
    typedef Edge8RelayArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    static_assert(DC >= 2 && DC <= 4, "columns of 2 .. 4 entries");
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_lds[];
    lds_f64 *X = (lds_f64 *)edge_lds;
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr uint64_t LOW = 0x0101010101010101ull;
    constexpr bool KEEP = R <= EDGE8_MEM_KEEP;

    double prv[R], msg[R], av[KEEP ? R : 1], gv[KEEP ? R : 1];
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
        {   // M = L0 (see bp_edge_relay_kernel)
            const auto l0_t = global_ptr(LDPC_EDGE_VARIANT_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // initialise_log_domain_bp (bp.hpp:147-157); phantom lanes: +inf
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
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

        double best = __builtin_inf();
        int nsol = 0, total = 0;
        const int legs = LDPC_KERNARG(ARGS_T, legs), stop_after = LDPC_KERNARG(ARGS_T, stop_after);
        const auto scol_t = global_ptr(LDPC_EDGE_VARIANT_ARG(scol));
        for (int leg = 0; leg < legs; ++leg) {
            const gtab_t a_t = global_ptr(LDPC_KERNARG(ARGS_T, ag_s)) + (size_t)leg * (2 * R * 64);  // the leg's tables: a, then gamma
            const gtab_t g_t = a_t + R * 64;
            const int leg_iters = global_ptr(LDPC_KERNARG(ARGS_T, leg_iters))[leg];
            const bool last = leg == legs - 1;
            if (KEEP) {
#pragma unroll
                for (int r = 0; r < R; ++r) { av[KEEP ? r : 0] = a_t[r * 64 + lane]; gv[KEEP ? r : 0] = g_t[r * 64 + lane]; }
            }
            if (leg > 0) {  // the initial messages of a later leg, from M = prv[r] (phantom lanes: a = +inf by gamma = 0)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double as = KEEP ? av[KEEP ? r : 0] : a_t[r * 64 + lane], gs = KEEP ? gv[KEEP ? r : 0] : g_t[r * 64 + lane];
                    msg[r] = gs == 0.0 ? as : as + gs * prv[r];
                }
            }

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
                // ---- bit pass (bp.hpp:276-318): the prior from M; the column's entries in order; log-ratio, decision, the lane's own bit_to_check; prv[r] <- the posterior ----
                uint64_t bad = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    double c[DC];
#pragma unroll
                    for (int j = 0; j < DC; ++j) c[j] = X[caddr[r][j]];
                    const double as = KEEP ? av[KEEP ? r : 0] : a_t[r * 64 + lane], gs = KEEP ? gv[KEEP ? r : 0] : g_t[r * 64 + lane];
                    if (!KEEP && (r & 1)) __builtin_amdgcn_sched_barrier(0);  // (two rounds' table reads in flight, not all R: they would cost 4 R registers)
                    const double pr = gs == 0.0 ? as : as + gs * prv[r];  // THIS iteration's prior, from M = prv[r]
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
                    prv[r] = t;  // M: the forward sum's end value, the same in every lane of the column
                }
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < leg_iters);
            total += it;

            // ---- the leg's end: a solution, or the last leg of a row without one (phantom lanes park theirs at the dummy slot behind +inf) ----
            LDPC_EDGE_RELAY_LEG_END(
                _Pragma("unroll") for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = prv[r];)
            if (nsol == stop_after) break;
        }
        {
            const auto ip = global_ptr(LDPC_EDGE_VARIANT_ARG(iters));
            const auto cp = global_ptr(LDPC_EDGE_VARIANT_ARG(conv));
            if (lane == 0) {
                if (ip) ip[b] = total;
                if (cp) cp[b] = nsol > 0 ? 1 : 0;
            }
        }
        __builtin_amdgcn_wave_barrier();  // (see bp_edge_kernel)
      }
        if (!work_pool_next(LDPC_EDGE_VARIANT_ARG(next), LDPC_EDGE_VARIANT_ARG(dyn_base), LDPC_EDGE_VARIANT_ARG(pool_per), LDPC_EDGE_VARIANT_ARG(chunk), (int)LDPC_EDGE_VARIANT_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_VARIANT_ARG(clk), clk_stamp);
}
#undef LDPC_EDGE_RELAY_LEG_END
