// bp_edge_rp_kernel.h -- bp_edge_rp_kernel, bp_edge8_rp_kernel: the lane = edge min-sum kernels with ROW PRIORS (every syndrome its own priors)
// Part of libldpc_hip.so: instantiated in tu_onchip_rp.hip, launched by host_onchip.h (decode_edge_rp, decode_edge8_rp).
#pragma once

#include "bp_edge_kernel.h"

// ldpc_hip_*_decode_batch_priors on a code of the lane = edge families (bp_edge_kernel.h): the general forms of bp_edge_kernel and
// bp_edge8_kernel (UNIFORM = false, NOCLAMP = false -- the clamp to DBL_MAX stays), on the same fragments (bp_edge_kernel.h), with ONE difference:
// the prior registers prv[r] are not filled once per kernel from EdgeArgs::prior_s but inside the syndrome loop, for the syndrome b the
// wavefront holds, from row b of `rowp` [batch][n] -- the log-ratios log((1 - P[b][j]) / P[b][j]) (io_kernels.h: row_priors_rowmajor_kernel,
// the operations of upload_priors) -- at the slot's column.  Row-major because a lane is an edge: the R loads of a wavefront for one
// syndrome touch the 8 n contiguous bytes of its row.  The slot's column is RE-READ per syndrome from the slot table (EdgeArgs::scol, 256 R
// bytes that stay in cache) rather than kept in R more registers: with it in registers bp_edge_rp_kernel<13 .. 16> and
// bp_edge8_rp_kernel<10, 3>, <12, 3>, <9, 4> spill (up to 32 VGPRs, 132 bytes of scratch a lane), and the two dependent loads a syndrome
// cost about a microsecond of the tens a wavefront spends on one.  A phantom lane is known by its partner address (the +inf slot) and gets
// the prior +inf, as in prior_s.
// The `0.0 + x` / `x + 0.0` argument of bp_edge_bit4.h / bp_edge_bit8.h holds as it does there: a row prior is log((1 - p) / p) by the same division and
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

// (LDPC_EDGE_ARG: bp_edge_kernel.h -- here the EdgeArgs / Edge8Args block is the member `e`)
#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, e.field)
#define LDPC_EDGE_PRIOR(r) prv[r]  // the prior of the bit-pass fragments: a register per lane and round

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
    constexpr int LG = 2;
    constexpr uint64_t LOW = 0x1111111111111111ull;
    constexpr bool NOCLAMP = false;  // (bp_edge_check4.h: the clamp to DBL_MAX stays)

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
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        // THIS syndrome's priors (b is wave-uniform: whichever row the wavefront pulled, never its slot's or its predecessor's)
        const auto pb = global_ptr(LDPC_KERNARG(ARGS_T, rowp)) + (int64_t)b * n;
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = paddr[r] == ZERO + 1 ? __builtin_inf() : pb[scol_t[r * 64 + lane]];  // phantom lanes: +inf (bp_edge_kernel.h); theirs is column 0 in the table
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = prv[r];  // initialise_log_domain_bp (bp.hpp:147-157)

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
            // ---- check pass: msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot ----
#include "bp_edge_check4.h"
            // ---- bit pass: the partner's message; log-ratio, decision, new bit_to_check ----
            uint64_t bad = 0;
#include "bp_edge_bit4.h"
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
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
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
    constexpr int LG = 3;
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

    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
        // THIS syndrome's priors (see bp_edge_rp_kernel)
        const auto pb = global_ptr(LDPC_KERNARG(ARGS_T, rowp)) + (int64_t)b * n;
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) prv[r] = caddr[r][0] == ZERO + 1 ? __builtin_inf() : pb[scol_t[r * 64 + lane]];  // phantom lanes (theirs is the dummy slot in the table): +inf
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = prv[r];  // initialise_log_domain_bp (bp.hpp:147-157); phantom lanes: +inf

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
            // ---- check pass (bp.hpp:220-273): minimum over the seven other lanes of the group, sign by the group's parity ----
#include "bp_edge_check8.h"
            // ---- bit pass (bp.hpp:276-318): the column's entries in order; log-ratio, decision, the lane's own bit_to_check ----
            uint64_t bad = 0;
#include "bp_edge_bit8.h"
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
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk), (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
}
#undef LDPC_EDGE_PRIOR
#undef LDPC_EDGE_ARG
