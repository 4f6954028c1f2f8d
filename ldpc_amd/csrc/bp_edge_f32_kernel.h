// bp_edge_f32_kernel.h -- bp_edge_f32_kernel, bp_edge8_f32_kernel: the lane = edge min-sum kernels of bp_edge_kernel.h with FP32 messages
// Part of libldpc_hip.so (instantiated in tu_onchip_f32.hip only; host side: host_onchip.h, decode_onchip_f32).
//
// The float32 message mode (ldpc_hip_bp_set_message_dtype) on the two code families the FP64 path serves with
// bp_edge_kernel (rows <= 4 in four neighbouring lanes, columns <= 2) and bp_edge8_kernel (rows <= 8 in eight lanes, columns <= DC): one
// wavefront per syndrome, a lane per edge and round, the edge's message in a register for the whole decode, check-to-bit messages exchanged
// through a wave-private LDS array -- everything as described at the top of bp_edge_kernel.h, restated for a 32-bit value: ONE DPP move per
// permutation, ONE v_cndmask per select, ds_*_b32, v_min_f32, R message registers per lane, 4 bytes per LDS slot.  The FP64 templates are
// not touched and not parametrised by the type.
//
// Reused as they are: the slot tables (partner / cpos, kind, scol: ensure_edge_tables, ensure_edge8_tables), the LDS slot convention
// (R * 64 slots, then +0.0, then +inf, then a dummy), work_pool_next, the clock probe, the lane-mask helpers of namespace edge_detail, and
// the two fragments of the FP64 kernels that touch no message: bp_edge_synd.h (a syndrome's bytes as lane masks) and bp_edge_out_status.h
// (`iters`, `conv`, the wave_barrier).  The passes have their own types throughout and stay written out here.
//
// Arithmetic: that of bp_f32_kernels.h and of tests/f32_util.py: min_sum_restatement(..., np.float32), which binds; per edge
//   priors       the handle's FP64 log((1 - p) / p) rounded ONCE to FP32, round-to-nearest-even (per slot: edge_prior_f32_kernel,
//                v_cvt_f32_f64; the UNIFORM form: the host's (float) of the same double); phantom lanes hold +inf.
//   check pass   magnitude = min over the OTHER entries of |bit_to_check| (FLT_MAX if there is none) -- min is exact and order-free, NaNs
//                are skipped as `abs < temp` skips them (v_min_f32 returns the other operand for a quiet NaN); sign = parity(syndrome byte
//                + #{entries <= 0}) + own; message = magnitude * (+-alpha) in ONE v_mul_f32; alpha is formed in FP64 (1 - ldexp(1, -it) for
//                ms_scaling_factor == 0) and rounded once to FP32, its sign applied by flipping the sign bit.
//   bit pass     column entries c0 (lower row), c1:  log-ratio = (prior + c0) + c1;
//                bit_to_check_0 = prior + (0.0 + c1), bit_to_check_1 = (prior + c0) + 0.0.
//                Both equal prior + (the other entry) EXACTLY: x + 0.0 differs from x only for x = -0.0, and neither
//                0.0 + c1 feeding a sum with the prior nor prior + c0 can be a -0.0 that matters -- the prior is
//                log((1 - p) / p), never -0.0, and a sum is -0.0 only if both terms are.  A column of weight one reads
//                a slot that holds +0.0 for good: prior + 0.0.  (The FP32 prior is never -0.0 either: the nonzero values of the FP64
//                log((1 - p) / p) are no smaller than 1.1e-16 -- (1 - p) / p is a double, next to 1.0 at best -- far above the least FP32
//                denormal, so the rounding never produces a zero that the double was not.)  Each sum is ONE v_add_f32.
// The restatement's minimum starts from FLT_MAX and replaces it only by something SMALLER: an infinite |bit_to_check| never enters it.
// Hence the clamp min(., FLT_MAX) after the butterfly -- and hence phantom lanes (a row lighter than four, the padding behind the last
// row) may hold +inf for good (prior +inf, partner = a slot that holds +inf): clamped to FLT_MAX in the minimum, positive in the sign
// ballot, and their "log-ratio" is +inf or, at worst, inf - inf = NaN: never <= 0, so they drop out of the decision ballots by themselves.
// Denormals are kept (the kernel descriptors say FP32 denormal mode 3: tu_onchip_f32.hip is built like every unit, without
// -fgpu-flush-denormals-to-zero) and nothing is contracted (the pragma below, and -ffp-contract=off in the Makefile).
// Outputs: decisions as bytes; the log-ratios as FP64, each the FP32 posterior widened exactly (v_cvt_f64_f32) by the lane that stores it.
#pragma once

#include "bp_edge_kernel.h"

#pragma clang fp contract(off)

struct EdgeF32Args {
    int32_t m, n, max_iter;
    double ms_scaling_factor;
    int64_t batch;
    const float *prior_s;      // [R * 64] prior of the slot's column; phantom: +inf          (general form)
    float prior_u;             // the one prior of every column                              (UNIFORM form: no prior registers)
    const uint16_t *partner;   // (as EdgeArgs: the FP64 kernel's table)
    int32_t chunk;
    int32_t static_per, dyn_base, pool_per;
    const uint8_t *kind;
    const int32_t *scol;
    const uint8_t *synd;       // [batch][m]
    uint8_t *decoding;         // [batch][n]
    double *llr;               // [batch][n] or nullptr: FP32 posteriors, widened
    int32_t *iters;            // [batch] or nullptr
    uint8_t *conv;             // [batch] or nullptr
    unsigned long long *next;
    unsigned long long *clk;
};

struct Edge8F32Args {
    int32_t m, n, max_iter;
    double ms_scaling_factor;
    int64_t batch;
    const float *prior_s;
    float prior_u;
    const uint16_t *cpos;      // (as Edge8Args)
    const uint8_t *kind;
    const int32_t *scol;
    int32_t chunk;
    int32_t static_per, dyn_base, pool_per;
    const uint8_t *synd;
    uint8_t *decoding;
    double *llr;
    int32_t *iters;
    uint8_t *conv;
    unsigned long long *next;
    unsigned long long *clk;
};

typedef void (*EdgeF32Kernel)(const EdgeF32Args);
typedef void (*Edge8F32Kernel)(const Edge8F32Args);
// The instantiations live in tu_onchip_f32.hip; the host side (host_onchip.h, in tu_onchip.hip) asks for them by the plan's numbers.
// nullptr: no such instantiation (the ladders are those of plan_edge and plan_edge8).
EdgeF32Kernel edge_f32_kernel(int rounds, bool uniform, bool noclamp);
Edge8F32Kernel edge8_f32_kernel(int rounds, int dc, bool uniform);

// The balance of scalar against vector work (see EDGE_V1 ... EDGE_G in bp_edge_kernel.h).  The FP32 kernels have their own constants; they
// start from the FP64 values and have not been retuned (no A/B on the GPU has been run for them yet).
#ifndef EDGE_F32_V1
#define EDGE_F32_V1 2
#endif
#ifndef EDGE_F32_V1N
#define EDGE_F32_V1N 8
#endif
#ifndef EDGE_F32_V2
#define EDGE_F32_V2 16
#endif
#ifndef EDGE_F32_G
#define EDGE_F32_G 4
#endif

// Resident wavefronts per SIMD an instantiation is compiled for (__launch_bounds__) and the host sizes its grid by (x 4 SIMDs per CU): the
// most that -Rpass-analysis=kernel-resource-usage shows without a VGPR spill (512 VGPRs per SIMD lane, granules of 8: 64 / 72 / 80 / 96 /
// 128 VGPRs for 8 / 7 / 6 / 5 / 4 wavefronts; DESIGN.md section 7a has the table) -- each instantiation was compiled at every level
// and takes the highest one it fits; bp_edge by R alone (its three forms fit the same level), bp_edge8 by R, DC and form.  The FP64
// kernels run 4 or 5.
__host__ __device__ constexpr int edge_f32_waves(int rounds) { return rounds <= 12 ? 8 : rounds <= 14 ? 7 : 6; }
__host__ __device__ constexpr int edge8_f32_waves(int rounds, int dc, bool uniform) {
    return dc == 3 ? (rounds <= 7 ? 8 : rounds == 8 ? (uniform ? 8 : 7) : rounds == 9 ? (uniform ? 7 : 6) : rounds == 10 ? (uniform ? 6 : 5) : 4)
                   : (rounds <= 4 ? 8 : rounds == 5 ? (uniform ? 8 : 7) : rounds == 6 ? 6 : rounds == 7 ? 5 : rounds == 8 ? (uniform ? 5 : 4) : 4);
}

#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, field)  // (bp_edge_kernel.h: the block is the arguments)

namespace edge_f32_detail {
using edge_detail::select_by_mask;
__device__ __forceinline__ int f2i(float x) { return __builtin_bit_cast(int, x); }
__device__ __forceinline__ float i2f(int x) { return __builtin_bit_cast(float, x); }
template <int CTRL>
__device__ __forceinline__ float quad_perm(float x) {  // ONE DPP move
    return i2f(__builtin_amdgcn_mov_dpp(f2i(x), CTRL, 0xf, 0xf, true));
}
// min(|a|, |b|) as ONE v_min_f32 with source modifiers; a quiet NaN operand yields the other operand, which is how
// `if (abs < temp) temp = abs` treats it
__device__ __forceinline__ float min_abs(float a, float b) {
    float r;
    asm("v_min_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float fmin_pos(float a, float uniform_b) {  // both >= +0 or NaN; the second from an SGPR
    float r;
    asm("v_min_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(uniform_b));
    return r;
}
__device__ __forceinline__ float uniform_f32(float x) { return i2f(__builtin_amdgcn_readfirstlane(f2i(x))); }  // wave-uniform value -> SGPR
__device__ __forceinline__ float select_f32(float a, float b, uint64_t mask) {  // per lane: bit `lane` of mask ? b : a -- ONE v_cndmask_b32
    return i2f(select_by_mask(f2i(a), f2i(b), mask));
}
// lane ^ 4 inside an 8-lane group: two DPP moves, each writing only the banks (groups of 4 lanes) it is right for
__device__ __forceinline__ float xor4(float x) {
    int v = __builtin_amdgcn_update_dpp(0, f2i(x), 0x104, 0xf, 0x5, false);   // row_shl:4 -> banks 0, 2 (lanes 0-3, 8-11)
    v = __builtin_amdgcn_update_dpp(v, f2i(x), 0x114, 0xf, 0xa, false);       // row_shr:4 -> banks 1, 3
    return i2f(v);
}
}  // namespace edge_f32_detail

// UNIFORM: all columns have the same prior (a decoder built from `error_rate`): it is a scalar, which frees R registers per lane; the
// phantom lanes' +inf then comes from their partner slot instead of their prior.
// NOCLAMP (with UNIFORM): the clamp to FLT_MAX cannot bite and is left out.  The host grants it (plan_edge, the FP64 kernel's conditions)
// when the prior is finite, |alpha| <= 1 and every row has at least two entries: then a real lane's minimum always covers a real entry,
// every message is bounded by (iterations + 1) x |prior| -- |check_to_bit| <= the largest |bit_to_check| of the round (|alpha| <= 1 after
// its rounding to FP32 too), |bit_to_check| <= |prior| + |check_to_bit| of its one partner -- and no infinity or NaN ever reaches a real
// lane.  In FP32 the bound must also stay below FLT_MAX for the clamp to be idle: a finite FP64 prior log((1 - p) / p) has |prior| <= 745
// (p down to the least denormal), and so has its FP32 rounding; max_iter is an int32, so (iterations + 1) x |prior| <= 2^31 x 745 < 1.7e12.
// The roundings do not lift that: a bit-to-check message is ONE correctly rounded sum of the prior and one message of magnitude B, and
// once B >= 2^34 half an ulp of B (2^10 at least) exceeds 745, so the sum rounds back to B -- the magnitudes never pass 2^34 + 2^11,
// 28 orders of magnitude below FLT_MAX ~ 3.4e38.  The phantom lanes' own infinities stay among themselves as before.
template <int R, bool UNIFORM, bool NOCLAMP = false>
__global__ void __launch_bounds__(64, edge_f32_waves(R)) bp_edge_f32_kernel(const EdgeF32Args a) {
    using namespace edge_detail;
    namespace f = edge_f32_detail;
    typedef EdgeF32Args ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_f32_lds[];
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f32 *X = (lds_f32 *)edge_f32_lds;  // [R * 64] check_to_bit of every slot, [R * 64] = +0.0 and [R * 64 + 1] = +inf for good
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr int LG = 2;
    constexpr uint64_t LOW = 0x1111111111111111ull;

    // per lane and round, for the whole kernel: prior, partner address; per round: which lanes are first / second entries
    float prv[UNIFORM ? 1 : R], msg[R];
    int paddr[R];
    uint64_t k0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
        if (!UNIFORM) prv[r] = a.prior_s[s];
        paddr[r] = (int)a.partner[s];
        k0[r] = __ballot(a.kind[s] == 1);
    }
    const float pu = f::uniform_f32(a.prior_u);
#define LDPC_EDGE_PRIOR(r) (UNIFORM ? pu : prv[UNIFORM ? 0 : (r)])
    const float flt_max = f::uniform_f32(FLT_MAX);
    if (lane == 0) { X[ZERO] = 0.0f; X[ZERO + 1] = __builtin_inff(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = UNIFORM ? (paddr[r] == ZERO + 1 ? __builtin_inff() : pu) : prv[r];  // every edge starts with its column's prior

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const float alpha = (float)((a.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.ms_scaling_factor);  // FP64, then one rounding
            const int ab = f::f2i(alpha), nb = ab ^ (int)0x80000000;
            // ---- check pass: msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot ----
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0f);
                const float x1 = f::quad_perm<0xB1>(cur);               // lane ^ 1
                const float pairmin = f::min_abs(cur, x1);
                const float other = f::quad_perm<0x4E>(pairmin);        // the other pair's minimum (lane ^ 2)
                const float mag = NOCLAMP ? f::min_abs(x1, other) : f::fmin_pos(f::min_abs(x1, other), flt_max);  // over the three other entries, from FLT_MAX down
                int sa;  // bits of +-alpha: sign = row parity (syndrome included) + own
                if (r < (NOCLAMP ? EDGE_F32_V1N : EDGE_F32_V1)) {
                    // the vector unit spreads the row's parity (see bp_edge_check4.h): 2 vector instructions more, 5 scalar ones fewer
                    const uint64_t par = nibble_parity_low(neg ^ sy[r]);
                    const int own = select_by_mask(ab, nb, neg);
                    const int rowbit = select_by_mask(0, (int)0x80000000, par);
                    sa = own ^ __builtin_amdgcn_mov_dpp(rowbit, 0x00, 0xf, 0xf, true);  // quad_perm [0, 0, 0, 0]
                } else {
                    const uint64_t flip = spread_nibble(nibble_parity_low(neg ^ sy[r])) ^ neg;  // row parity incl. the syndrome, own sign out
                    sa = select_by_mask(ab, nb, flip);
                }
                const float c = mag * f::i2f(sa);
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
            // ---- bit pass: the partner's message; log-ratio, decision, new bit_to_check ----
            uint64_t bad = 0;
            // (groups of EDGE_F32_G rounds: their LDS reads are issued together, then consumed -- one round trip per group, not per round)
#pragma unroll
            for (int r0 = 0; r0 < R; r0 += EDGE_F32_G) {
                float cpv[EDGE_F32_G];
#pragma unroll
                for (int g = 0; g < EDGE_F32_G; ++g)
                    if (r0 + g < R) cpv[g] = X[paddr[r0 + g]];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < EDGE_F32_G; ++g) {
                    const int r = r0 + g;
                    if (r >= R) break;
                    const float cp = cpv[g];
                    const float c = msg[r];
                    const float b2c = LDPC_EDGE_PRIOR(r) + cp;
                    const float l1 = b2c + c;                       // second entry of its column: (prior + c0) + c1 with c0 = the partner's
                    const float l0 = (LDPC_EDGE_PRIOR(r) + c) + cp; // first entry: c0 = its own
                    uint64_t d;
                    if (r < EDGE_F32_V2) {  // the vector unit picks the lane's own log-ratio: 1 vector instruction more, 3 scalar ones fewer
                        d = __ballot(f::select_f32(l1, l0, k0[r]) <= 0.0f);
                    } else {
                        const uint64_t d1 = __ballot(l1 <= 0.0f);
                        d = d1 ^ ((__ballot(l0 <= 0.0f) ^ d1) & k0[r]);  // (phantom lanes: neither)
                    }
                    bad |= nibble_parity_low(d) ^ sy[r];  // candidate syndrome vs syndrome, bit 0 of every nibble
                    msg[r] = b2c;
                }
            }
            unsat = never || (bad & LOW) != 0;
        } while (unsat && it < a.max_iter);

        // ---- outputs: the log-ratios, formed from the last iteration's messages by the lanes that own the first entry of a column,
        //      change places with the messages (X[j] = log-ratio of column j; n <= R * 64: every column has an entry, and the next
        //      syndrome's first check pass rewrites every slot), then leave in whole rows, widened to FP64 on the way ----
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = (LDPC_EDGE_PRIOR(r) + X[r * 64 + lane]) + X[paddr[r]];
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = scol_t[r * 64 + lane];
            if ((k0[r] >> lane) & 1ull) X[j] = msg[r];
        }
        {
            const auto dp = global_ptr(LDPC_EDGE_ARG(decoding)) + (int64_t)b * n;
            auto lp = global_ptr(LDPC_EDGE_ARG(llr));
            if (lp) lp += (int64_t)b * n;
            for (int j = lane; j < n; j += 64) {
                const float l0 = X[j];
                dp[j] = l0 <= 0.0f ? 1 : 0;
                if (lp) lp[j] = (double)l0;
            }
        }
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk),
                            (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
#undef LDPC_EDGE_PRIOR
}

// ---- heavier nodes: rows of weight <= 8 in EIGHT neighbouring lanes, columns of weight <= DC (<= 4) -- bp_edge8_kernel in FP32 ----
// A lane reads ALL entries of its column from the wave-private LDS array in column order (lighter columns: the +0.0 slot behind their
// entries) and forms the restatement's sums with them:
//     log-ratio            (((prior + c0) + c1) + c2) + c3, the same in every lane of a column,
//     bit_to_check of k    ((prior + c0) + ... + c_{k-1})  +  (((0 + c_{DC-1}) + ...) + c_{k+1})
// (0.0 + x and x + 0.0 are dropped where x + a prior follows or the sum contains the prior: they can only turn -0.0 into +0.0, which a
// sum with a prior log((1-p)/p) -- never -0.0 -- does not see); the lane's own k picks its bit_to_check by two or three v_cndmask reading
// per-round lane masks from SGPRs.
template <int R, int DC, bool UNIFORM>
__global__ void __launch_bounds__(64, edge8_f32_waves(R, DC, UNIFORM)) bp_edge8_f32_kernel(const Edge8F32Args a) {
    using namespace edge_detail;
    namespace f = edge_f32_detail;
    typedef Edge8F32Args ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    static_assert(DC >= 2 && DC <= 4, "columns of 2 .. 4 entries");
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_f32_lds[];
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f32 *X = (lds_f32 *)edge_f32_lds;
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr int LG = 3;
    constexpr uint64_t LOW = 0x0101010101010101ull;

    float prv[UNIFORM ? 1 : R], msg[R];
    int caddr[R][DC];
    uint64_t kmask[R][DC - 1];  // lanes whose entry is the (j + 1)-th of its column, j < DC - 1
    bool phantom_lane[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
        if (!UNIFORM) prv[r] = a.prior_s[s];
#pragma unroll
        for (int j = 0; j < DC; ++j) caddr[r][j] = (int)a.cpos[(size_t)j * (R * 64) + s];
        const int kd = a.kind[s];
        phantom_lane[r] = kd == 0;
#pragma unroll
        for (int j = 0; j < DC - 1; ++j) kmask[r][j] = __ballot(kd == j + 2);
    }
    const float pu = f::uniform_f32(a.prior_u);
#define LDPC_EDGE_PRIOR(r) (UNIFORM ? pu : prv[UNIFORM ? 0 : (r)])
    const float flt_max = f::uniform_f32(FLT_MAX);
    if (lane == 0) { X[ZERO] = 0.0f; X[ZERO + 1] = __builtin_inff(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = phantom_lane[r] ? __builtin_inff() : LDPC_EDGE_PRIOR(r);  // every edge starts with its column's prior

        int it = 0;
        bool unsat = true;
        do {
            ++it;
            const float alpha = (float)((a.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.ms_scaling_factor);  // FP64, then one rounding
            const int ab = f::f2i(alpha), nb = ab ^ (int)0x80000000;
            // ---- check pass: minimum over the seven other lanes of the group, sign by the group's parity ----
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float cur = msg[r];
                const uint64_t neg = __ballot(cur <= 0.0f);
                const float x1 = f::quad_perm<0xB1>(cur);                // lane ^ 1
                const float pairmin = f::min_abs(cur, x1);
                const float otherpair = f::quad_perm<0x4E>(pairmin);     // lane ^ 2: the other pair of the quad
                const float inquad = f::min_abs(x1, otherpair);          // the three others of the quad
                const float quadmin = f::min_abs(pairmin, otherpair);    // ... and the whole quad, for the other quad (values >= 0: |.| is idle)
                const float otherquad = f::xor4(quadmin);
                const float mag = f::fmin_pos(f::min_abs(inquad, otherquad), flt_max);  // the seven other entries, from FLT_MAX down
                const uint64_t flip = spread_byte(byte_parity_low(neg ^ sy[r])) ^ neg;
                const float c = mag * f::i2f(select_by_mask(ab, nb, flip));
                msg[r] = c;
                X[r * 64 + lane] = c;
            }
            // ---- bit pass: the column's entries in order; log-ratio, decision, the lane's own bit_to_check ----
            uint64_t bad = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float c[DC];
#pragma unroll
                for (int j = 0; j < DC; ++j) c[j] = X[caddr[r][j]];
                const float pr = LDPC_EDGE_PRIOR(r);
                float pre[DC];  // pre[k] = prior + c0 + ... + c_{k-1}
                float t = pr;
#pragma unroll
                for (int j = 0; j < DC; ++j) { pre[j] = t; t += c[j]; }
                const uint64_t d = __ballot(t <= 0.0f);  // (phantom lanes: +inf or NaN, never <= 0)
                bad |= byte_parity_low(d) ^ sy[r];
                // the lane's own bit_to_check: cand[k] = pre[k] + (((0 + c_{DC-1}) + ...) + c_{k+1}), accumulated downwards as the
                // restatement does; the k-th entry of its column takes cand[k]
                float cand[DC];
                float sfx = c[DC - 1];
                cand[DC - 1] = pre[DC - 1];
                cand[DC - 2] = pre[DC - 2] + sfx;
#pragma unroll
                for (int k = DC - 3; k >= 0; --k) { sfx += c[k + 1]; cand[k] = pre[k] + sfx; }
                float b2c = cand[0];
#pragma unroll
                for (int k = 1; k < DC; ++k) b2c = f::select_f32(b2c, cand[k], kmask[r][k - 1]);
                msg[r] = b2c;
            }
            unsat = never || (bad & LOW) != 0;
        } while (unsat && it < a.max_iter);

        // ---- outputs: as bp_edge_f32_kernel -- every lane of a column holds the column's log-ratio (the same bits) and parks it at
        //      X[column] (phantom lanes: at the dummy slot behind +inf), then whole rows leave ----
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float t = LDPC_EDGE_PRIOR(r);
#pragma unroll
            for (int j = 0; j < DC; ++j) t += X[caddr[r][j]];
            msg[r] = t;
        }
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = msg[r];
        {
            const auto dp = global_ptr(LDPC_EDGE_ARG(decoding)) + (int64_t)b * n;
            auto lp = global_ptr(LDPC_EDGE_ARG(llr));
            if (lp) lp += (int64_t)b * n;
            for (int j = lane; j < n; j += 64) {
                const float t = X[j];
                dp[j] = t <= 0.0f ? 1 : 0;
                if (lp) lp[j] = (double)t;
            }
        }
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk),
                            (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
#undef LDPC_EDGE_PRIOR
}
#undef LDPC_EDGE_ARG
