// bp_edge_relay_kernel.h -- bp_edge_relay_kernel, bp_edge8_relay_kernel: Relay-BP on the lane = edge min-sum kernels, all legs of a syndrome in one launch
// Part of libldpc_hip.so: instantiated in tu_onchip_relay.hip, launched by host_onchip.h (decode_edge_relay, decode_edge8_relay).
#pragma once

#include "bp_edge_mem_kernel.h"
#include "relay_common.h"

// ldpc_hip_bp_set_relay on a code of the lane = edge families: the check and bit passes of bp_edge_mem_kernel / bp_edge8_mem_kernel
// (bp_edge_mem_kernel.h) -- the same fragments (bp_edge_kernel.h) -- inside a loop over the legs -- one wavefront per syndrome, M in the registers prv[r], nothing
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

// (LDPC_EDGE_ARG: bp_edge_kernel.h -- here the EdgeArgs / Edge8Args block is the member `e`)
#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, e.field)

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
    constexpr int LG = 2;
    constexpr uint64_t LOW = 0x1111111111111111ull;
    constexpr bool NOCLAMP = false;  // (bp_edge_check4.h: the clamp to DBL_MAX stays)
    constexpr bool KEEP = R <= EDGE_MEM_KEEP;

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
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        {   // M = L0: leg 0's initial messages (initialise_log_domain_bp, bp.hpp:147-157), and what its first iteration's prior is formed from
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // (phantom lanes: +inf)
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
#include "bp_edge_synd.h"  // sy[r], never

        double best = __builtin_inf();
        int nsol = 0, total = 0;
        const int legs = LDPC_KERNARG(ARGS_T, legs), stop_after = LDPC_KERNARG(ARGS_T, stop_after);
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
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
#include "bp_edge_check4.h"
                // ---- bit pass: the prior from M; the partner's message; log-ratio, decision, new bit_to_check; prv[r] <- the column's posterior ----
                uint64_t bad = 0;
#include "bp_edge_bit4_mem.h"
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < leg_iters);
            total += it;

            // ---- the leg's end: a solution, or the last leg of a row without one (the first entry of a column parks the column's log-ratio) ----
            if (!unsat || (last && nsol == 0)) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int j = scol_t[r * 64 + lane];
                    if ((k0[r] >> lane) & 1ull) X[j] = prv[r];
                }
#include "bp_edge_relay_take.h"
            }
            if (nsol == stop_after) break;
        }
        {   // iters = the iterations of all legs run, conv = a solution was found
            const int it = total;
            const bool unsat = !(nsol > 0);
#include "bp_edge_out_status.h"
        }
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
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
    constexpr int LG = 3;
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

    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        {   // M = L0 (see bp_edge_relay_kernel)
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // initialise_log_domain_bp (bp.hpp:147-157); phantom lanes: +inf
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
#include "bp_edge_synd.h"  // sy[r], never

        double best = __builtin_inf();
        int nsol = 0, total = 0;
        const int legs = LDPC_KERNARG(ARGS_T, legs), stop_after = LDPC_KERNARG(ARGS_T, stop_after);
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
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
#include "bp_edge_check8.h"
                // ---- bit pass (bp.hpp:276-318): the prior from M; the column's entries in order; log-ratio, decision, the lane's own bit_to_check; prv[r] <- the posterior ----
                uint64_t bad = 0;
#include "bp_edge_bit8.h"
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < leg_iters);
            total += it;

            // ---- the leg's end: a solution, or the last leg of a row without one (phantom lanes park theirs at the dummy slot behind +inf) ----
            if (!unsat || (last && nsol == 0)) {
#pragma unroll
                for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = prv[r];
#include "bp_edge_relay_take.h"
            }
            if (nsol == stop_after) break;
        }
        {   // iters = the iterations of all legs run, conv = a solution was found
            const int it = total;
            const bool unsat = !(nsol > 0);
#include "bp_edge_out_status.h"
        }
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
}
#undef LDPC_EDGE_ARG
