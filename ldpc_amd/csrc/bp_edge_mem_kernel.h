// bp_edge_mem_kernel.h -- bp_edge_mem_kernel, bp_edge8_mem_kernel: the lane = edge min-sum kernels with MEMORY (per-bit memory strengths)
// Part of libldpc_hip.so: instantiated in tu_onchip_mem.hip, launched by host_onchip.h (decode_edge_mem, decode_edge8_mem).
#pragma once

#include "bp_edge_kernel.h"

// ldpc_hip_bp_set_memory on a code of the lane = edge families (bp_edge_kernel.h): the general forms of bp_edge_kernel and bp_edge8_kernel
// (UNIFORM = false, NOCLAMP = false -- the clamp to DBL_MAX stays), on the same fragments (bp_edge_kernel.h), with ONE difference: the prior registers
// prv[r] hold M, and every bit pass forms its prior from them -- from the posterior of the lane's column that the previous bit pass formed:
//     prior = gamma == 0 ? a : a + gamma * M           (the product rounded, then the sum: -ffp-contract=off)
// with M the column's posterior of the previous iteration (the prior log-ratio L0 before the first), a = (1 - gamma) * L0 formed on the
// host (mem_host.h) and a = L0 itself where gamma == 0 -- so the select needs no third table.  Every lane of a column forms the SAME posterior
// -- (prior + c0) + c1 (+ c2 + c3) in the column's order, from the same prior -- hence the same prior again: by induction the lanes of a column
// never disagree, and M is one more register per round, not an exchange.  The initial messages are L0 (EdgeArgs::prior_s), as in the plain kernel.
// a and gamma come per slot from slot tables (EdgeMemArgs::a_s, g_s; edge_mem_table_kernel, host_onchip.h).  Up to KEEP rounds they stay in
// registers for the whole kernel; above, they are RE-READ in every bit pass (512 R bytes a table that stay in cache), a few rounds at a time
// beside the LDS reads of the same rounds, as the row-prior kernels re-read scol: with them in registers the higher instantiations spill.  A phantom lane has a = +inf and gamma = 0: its prior stays +inf.
// The `0.0 + x` / `x + 0.0` argument of bp_edge_bit4.h / bp_edge_bit8.h holds as it does there.  It needs a prior that is never -0.0: a is never -0.0
// (mem_host.h: 1 - gamma >= 2^-53 and |L0| >= 1.1e-16 or L0 = +0.0, the product neither underflows nor changes sign), and a sum is -0.0 only if
// BOTH terms are -- so a + gamma * M is not, whatever gamma * M is (a - a is +0.0 in round-to-nearest).  With the prior not -0.0, no
// prior + c0 (+ ...) is -0.0 either, and 0.0 + c feeding a sum with one of those cannot matter.
// Results are bit-identical to the per-pass memory kernels (bp_spread_kernels.h: bp_spread_mem_*) and to the NumPy restatement (tests/mem_bp_util.py).
struct EdgeMemArgs {
    EdgeArgs e;           // prior_s: L0 per slot (the initial messages and M); prior_u: not read
    const double *a_s;    // [R * 64] a of the slot's column; phantom: +inf
    const double *g_s;    // [R * 64] gamma of the slot's column; phantom: 0
};
struct Edge8MemArgs {
    Edge8Args e;
    const double *a_s;
    const double *g_s;
};

typedef void (*EdgeMemKernel)(const EdgeMemArgs);
typedef void (*Edge8MemKernel)(const Edge8MemArgs);
// The instantiations live in tu_onchip_mem.hip; the host side (host_onchip.h, in tu_onchip.hip) asks for them by the plan's numbers.
// nullptr: no such instantiation (the ladders are those of plan_edge and plan_edge8).
EdgeMemKernel edge_mem_kernel(int rounds);
Edge8MemKernel edge8_mem_kernel(int rounds, int dc);

// rounds up to which a and gamma stay in registers (above: re-read per bit pass), and the wavefronts per SIMD the instantiations are compiled
// for -- the host sizes its grid by them (launch_edge_mem).  bp_edge_mem_kernel<14 .. 16> spill 12 .. 38 VGPRs at four (128 registers: M, the
// message and the partner address of 14 rounds are 70 of them, the table reads of a group 16 more) and get three (168); nothing else spills
// or uses scratch.  What each instantiation compiles to is listed in DESIGN.md section 7c.
#ifndef EDGE_MEM_KEEP
#define EDGE_MEM_KEEP 8
#endif
#ifndef EDGE8_MEM_KEEP
#define EDGE8_MEM_KEEP 5
#endif

__host__ __device__ constexpr int edge_mem_waves(int rounds) { return rounds <= 13 ? 4 : 3; }
__host__ __device__ constexpr int edge8_mem_waves(int, int) { return 4; }

// (LDPC_EDGE_ARG: bp_edge_kernel.h -- here the EdgeArgs / Edge8Args block is the member `e`)
#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, e.field)

template <int R>
__global__ void __launch_bounds__(64, edge_mem_waves(R)) bp_edge_mem_kernel(const EdgeMemArgs ma) {
    using namespace edge_detail;
    const EdgeArgs &a = ma.e;
    typedef EdgeMemArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
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

    // per lane and round, for the whole kernel: partner address, (KEEP) a and gamma; per round: which lanes are first entries.  prv[r]: per ITERATION
    double prv[R], msg[R], av[KEEP ? R : 1], gv[KEEP ? R : 1];
    int paddr[R];
    uint64_t k0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
        paddr[r] = (int)a.partner[s];
        k0[r] = __ballot(a.kind[s] == 1);
        if (KEEP) { av[r] = ma.a_s[s]; gv[r] = ma.g_s[s]; }
    }
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        const gtab_t a_t = KEEP ? (gtab_t)nullptr : global_ptr(LDPC_KERNARG(ARGS_T, a_s));  // (re-read per iteration above KEEP rounds)
        const gtab_t g_t = KEEP ? (gtab_t)nullptr : global_ptr(LDPC_KERNARG(ARGS_T, g_s));
        {   // M = L0: the initial messages (initialise_log_domain_bp, bp.hpp:147-157), and what the first iteration's prior is formed from
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // (phantom lanes: +inf)
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
#include "bp_edge_synd.h"  // sy[r], never

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
        } while (unsat && it < a.max_iter);

        // ---- outputs (as bp_edge_kernel): the first entry of a column parks the column's log-ratio at X[column], whole rows leave.  The log-ratio
        // is prv[r], formed by the last bit pass (the plain kernel adds it up again from the prior; that prior is history here) ----
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = scol_t[r * 64 + lane];
            if ((k0[r] >> lane) & 1ull) X[j] = prv[r];
        }
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
}

template <int R, int DC>
__global__ void __launch_bounds__(64, edge8_mem_waves(R, DC)) bp_edge8_mem_kernel(const Edge8MemArgs ma) {
    using namespace edge_detail;
    const Edge8Args &a = ma.e;
    typedef Edge8MemArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
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
        if (KEEP) { av[r] = ma.a_s[s]; gv[r] = ma.g_s[s]; }
    }
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        const gtab_t a_t = KEEP ? (gtab_t)nullptr : global_ptr(LDPC_KERNARG(ARGS_T, a_s));  // (re-read per iteration above KEEP rounds)
        const gtab_t g_t = KEEP ? (gtab_t)nullptr : global_ptr(LDPC_KERNARG(ARGS_T, g_s));
        {   // M = L0 (see bp_edge_mem_kernel)
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) msg[r] = l0_t[r * 64 + lane];  // initialise_log_domain_bp (bp.hpp:147-157); phantom lanes: +inf
        }
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = msg[r];
#include "bp_edge_synd.h"  // sy[r], never

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
        } while (unsat && it < a.max_iter);

        // ---- outputs: as bp_edge8_kernel, with the log-ratio the last bit pass formed (phantom lanes park theirs at the dummy slot behind +inf) ----
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = prv[r];
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
}
#undef LDPC_EDGE_ARG
