// bp_edge_kernel.h -- bp_edge_kernel: min-sum with LANE = EDGE and the messages in REGISTERS (BASELINE config 3)
// Part of libldpc_hip.so (one translation unit: bp_hip.hip includes every kernel header).
#pragma once

#include "bp_device_common.h"

// For the codes of the surface-code family -- rows of weight <= 4, columns of weight <= 2 (rotated / toric surface codes,
// ring codes) -- the node-per-lane kernel (bp_wave_kernel.h) spends ~745 wave-instructions per syndrome-iteration on 840
// edges: address arithmetic, position-table reads, a separate syndrome sweep, every message through LDS twice per pass.
// Here a wavefront still owns one syndrome, but
//   * a LANE owns one EDGE per round (slot s = 64 r + lane, r < R rounds), and a row's (up to) four edges sit in four
//     neighbouring lanes (slot = 4 i + k): the check update (bp.hpp:220-273) needs the other entries of the row -- two
//     DPP quad permutations -- and the row's sign parity -- one ballot and scalar bit tricks on the 64-bit lane mask;
//   * the edge's message lives in a REGISTER for the whole decode (R of them per lane); the bit update (bp.hpp:276-318)
//     needs the one other entry of the column, which sits in some other lane and round: every lane stores its
//     check-to-bit message at its own slot of a wave-private LDS array and reads its partner's (2 LDS operations per edge
//     and iteration instead of 8, and no index tables: the partner's address is a register);
//   * hard decisions never leave the scalar unit: ballots of (log-ratio <= 0), nibble parities, XOR with the syndrome mask.
// Arithmetic, per edge and in the reference's association:
//   check pass   magnitude = min over the OTHER entries of |bit_to_check| (DBL_MAX if there is none) -- min is exact and
//                order-free, NaNs are skipped as `abs < temp` skips them (bp.hpp:241-247, :257-259, :268-270; v_min_f64
//                returns the other operand for a quiet NaN); sign = parity(syndrome byte + #{entries <= 0}) + own
//                (bp.hpp:236-262); message = magnitude * (+-alpha) (bp.hpp:264-266).
//   bit pass     column entries c0 (lower row), c1:  log-ratio = (prior + c0) + c1 (bp.hpp:278-281);
//                bit_to_check = prior + (the other entry), which is the reference's sum EXACTLY.
// Results are bit-identical to bp_wave_kernel and to the reference (tests/test_gpu_parity.py, test_gpu_fuzz.py).
// The variants (bp_edge_rp_kernel.h: row priors, bp_edge_mem_kernel.h: memory, bp_edge_relay_kernel.h: Relay-BP, bp_edge_gd_kernel.h: guided
// decimation) run the SAME passes, and every pass is written once, in a textual fragment that the kernels #include where the pass stands:
//   bp_edge_check4.h, bp_edge_check8.h   the check pass, rows in four / eight lanes (the clamp to DBL_MAX, the phantom lanes, the DPP parity spread)
//   bp_edge_bit4.h, bp_edge_bit4_mem.h   the bit pass for columns of weight <= 2, plain / memory form (-0.0, the grouped LDS reads)
//   bp_edge_bit8.h                       the bit pass for columns of weight <= DC, both forms
//   bp_edge_synd.h                       a syndrome's bytes as lane masks
//   bp_edge_out_rows.h, bp_edge_out_status.h   the outputs leave; the wave_barrier at the end of a syndrome's turn
// Each fragment's header lists the names it takes from the kernel, and carries the argument for its code, once.  Textual because a fragment
// gives every kernel the token stream it had with the pass written out, hence the same code (profiles/edge_fragments_isa.txt); as
// __forceinline__ function templates -- whole passes on the register arrays, or one round on values -- the passes compiled to other
// instruction streams in many instantiations (profiles/edge_passes_isa.txt).  Still written out in each kernel: the table set-up and the
// work loop (two halves that bracket the kernel; edge_fragments_isa.txt says why).  Shared as code: edge_detail below, the two ladders, and
// ONE launch on the host (launch_edge, host_onchip.h).
struct EdgeArgs {
    int32_t m, n, max_iter;
    double ms_scaling_factor;
    int64_t batch;
    const double *prior_s;     // [R * 64] prior of the slot's column; phantom: +inf          (general form)
    double prior_u;            // the one prior of every column                              (UNIFORM form: no prior registers)
    const uint16_t *partner;   // [R * 64] slot of the other entry of the slot's column; none: R * 64 (the +0.0 slot); a phantom lane:
                               // R * 64 + 1 (a slot that holds +inf for good)
    int32_t chunk;             // syndromes pulled per visit to a work counter
    int32_t static_per, dyn_base, pool_per;  // work_pool_next: static share per wavefront, where the pools start, syndromes per pool (batch < 2^30)
    const uint8_t *kind;       // [R * 64] 0 phantom, 1 first entry of its column (lower row), 2 second entry
    const int32_t *scol;       // [R * 64] column of the slot (outputs are written by the kind-1 lanes)
    const uint8_t *synd;       // [batch][m]
    uint8_t *decoding;         // [batch][n]
    double *llr;               // [batch][n] or nullptr
    int32_t *iters;            // [batch] or nullptr
    uint8_t *conv;             // [batch] or nullptr
    unsigned long long *next;  // WORK_POOLS work counters, WORK_POOL_STRIDE words apart (work_pool_next, bp_device_common.h) (zeroed before launch)
    unsigned long long *clk;   // shader-clock probe (clock_probe_*, bp_device_common.h) or nullptr
};

// The instantiations of the two families, written once: bp_edge_kernel and its variants exist for LDPC_EDGE_LADDER's rounds (plan_edge,
// host_onchip.h, takes the code's own (4 m + 63) / 64), bp_edge8_kernel and its variants for LDPC_EDGE8_LADDER's (rounds, column weight) rungs
// (plan_edge8 takes the first of its column weight that holds 8 m slots: they ascend).  X is applied to every rung.
#define LDPC_EDGE_LADDER(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define LDPC_EDGE8_LADDER(X)                                                             \
    X(2, 3) X(3, 3) X(4, 3) X(5, 3) X(6, 3) X(7, 3) X(8, 3) X(9, 3) X(10, 3) X(12, 3) \
    X(2, 4) X(3, 4) X(4, 4) X(5, 4) X(6, 4) X(7, 4) X(8, 4) X(9, 4)

__host__ __device__ inline size_t edge_lds_bytes(int rounds) { return ((size_t)rounds * 64 + 3) * 8; }  // slots, +0.0, +inf, a dummy (bp_edge8_kernel's phantom lanes park their output there)
__host__ __device__ inline size_t edge_f32_lds_bytes(int rounds) { return ((size_t)rounds * 64 + 3) * 4; }  // the same slots at 4 bytes each (bp_edge_f32_kernel.h)

// How many of the R rounds let the vector unit do what the scalar unit would (both issue one instruction per SIMD turn, and the
// kernel's scalar work -- lane-mask parities -- outweighs its vector work): measured on BASELINE config 3, tools/bench_edge.py
// (C3, M syndromes/s: none 60.9; V2 all rounds 64.3; V1 all rounds 62.0; both 66.1; V1 = 2 rounds + V2 all 66.8)
#ifndef EDGE_V1
#define EDGE_V1 2
#endif
#ifndef EDGE_V1N  // ... in the form without the clamp (one vector instruction a round fewer: the balance moves; C3, M syndromes/s, x3 on one box:
#define EDGE_V1N 8  //     2: 65.7;  3: 66.2;  4: 66.2;  6: 66.7;  8: 66.7;  10: 66.3;  14: 66.3 -- flat from 6 up, profiles/r6_c3_noclamp_ab.txt)
#endif
#ifndef EDGE_V2
#define EDGE_V2 16
#endif
#ifndef EDGE_G
#define EDGE_G 4
#endif
// LDPC_EDGE_ARG(field): a cold field (LDPC_KERNARG, bp_device_common.h) of the EdgeArgs / Edge8Args block in a kernel's arguments ARGS_T -- the
// one spelling the kernels and the fragments use.  Every kernel header defines it for its own kernels and undefines it at its end: here the
// block IS the arguments; in a variant it is their member `e`, and the variant's own fields are LDPC_KERNARG(ARGS_T, field).
#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, field)
namespace edge_detail {
typedef __attribute__((address_space(3))) double lds_f64;         // the wave-private LDS array of messages
typedef __attribute__((address_space(1))) const double *gtab_t;  // a slot table of doubles in global memory
// quad permutations of a double (two 32-bit DPP moves: 64-bit DPP allows row_newbcast only)
template <int CTRL>
__device__ __forceinline__ double quad_perm(double x) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// min(|a|, |b|) as ONE v_min_f64 with source modifiers (fmin() would first canonicalise both operands: two more instructions);
// a quiet NaN operand yields the other operand, which is how `if (abs < temp) temp = abs` treats it
__device__ __forceinline__ double min_abs(double a, double b) {
    double r;
    asm("v_min_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double fmin_pos(double a, double uniform_b) {  // both >= +0 or NaN; the second from an SGPR pair
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(uniform_b));
    return r;
}
// per lane: bit `lane` of the wave-uniform mask selects b, else a -- one v_cndmask_b32 reading the mask from an SGPR pair
__device__ __forceinline__ int select_by_mask(int a, int b, uint64_t mask) {
    int r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}
__device__ __forceinline__ double uniform_f64(double x) {  // wave-uniform value -> SGPR pair
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// every bit of a nibble := XOR of the nibble's four bits (a row's four lanes)
__device__ __forceinline__ uint64_t nibble_parity_low(uint64_t x) {  // result in bit 0 of every nibble; the other bits are garbage
    x ^= x >> 1;
    x ^= x >> 2;
    return x;
}
__device__ __forceinline__ uint64_t spread_nibble(uint64_t low) {  // bit 0 of every nibble -> all four bits
    const uint32_t a = ((uint32_t)low & 0x11111111u) * 15u, b = ((uint32_t)(low >> 32) & 0x11111111u) * 15u;
    return ((uint64_t)b << 32) | a;
}
// +-alpha of iteration `it` as words -- the low word, the high word, the high word of -alpha: a check pass multiplies the magnitude by the double
// it puts together from `lo` and one of the high words (scaling factor 0: the adaptive 1 - 2^-it, bp.hpp:264-266)
struct AlphaWords { int lo, hi, nhi; };
__device__ __forceinline__ AlphaWords alpha_words(double ms_scaling_factor, int it) {
    const double alpha = (ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : ms_scaling_factor;
    const int ahi = __double2hiint(alpha);
    return {__double2loint(alpha), ahi, ahi ^ (int)0x80000000};
}
}  // namespace edge_detail

// UNIFORM: all columns have the same prior (a decoder built from `error_rate`): it is a scalar, which frees 2 R registers per
// lane -- a fifth resident wavefront per SIMD; the phantom lanes' +inf then comes from their partner slot instead of their prior.
// NOCLAMP (with UNIFORM): the clamp to DBL_MAX cannot bite and is left out (one vector instruction of ~19 per round, and the kernel is bound
// by vector issue).  The host grants it (plan_edge) when the prior is finite, |alpha| <= 1 and every row has at least two entries: then a
// real lane's minimum always covers a real entry, every message is bounded by (iterations + 1) x |prior| -- |check_to_bit| <= the largest
// |bit_to_check| of the round, |bit_to_check| <= |prior| + |check_to_bit| of its one partner -- and no infinity or NaN ever reaches a real
// lane; the phantom lanes' own infinities stay among themselves as before (inf - inf = NaN is not <= 0 either).
template <int R, bool UNIFORM, bool NOCLAMP = false>
__global__ void __launch_bounds__(64, UNIFORM ? 5 : 4) bp_edge_kernel(const EdgeArgs a) {
    using namespace edge_detail;
    typedef EdgeArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_lds[];
    lds_f64 *X = (lds_f64 *)edge_lds;  // [R * 64] check_to_bit of every slot, [R * 64] = +0.0 for good
    const int lane = threadIdx.x;
    __shared__ unsigned long long clk_stamp[2];
    if (lane == 0) clock_probe_begin(clk_stamp);
    const int m = a.m, n = a.n;
    constexpr int ZERO = R * 64;
    constexpr int LG = 2;  // a row sits in 1 << LG neighbouring lanes; LOW: bit 0 of every such group
    constexpr uint64_t LOW = 0x1111111111111111ull;

    // per lane and round, for the whole kernel: prior, partner address; per round: which lanes are first / second entries
    double prv[UNIFORM ? 1 : R], msg[R];
    int paddr[R];
    uint64_t k0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int s = r * 64 + lane;
        if (!UNIFORM) prv[r] = a.prior_s[s];
        paddr[r] = (int)a.partner[s];
        k0[r] = __ballot(a.kind[s] == 1);
    }
    const double pu = uniform_f64(a.prior_u);
#define LDPC_EDGE_PRIOR(r) (UNIFORM ? pu : prv[UNIFORM ? 0 : (r)])
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = UNIFORM ? (paddr[r] == ZERO + 1 ? __builtin_inf() : pu) : prv[r];  // initialise_log_domain_bp (bp.hpp:147-157)

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

        // ---- outputs (bp.hpp:62,65,69,71): the log-ratios, formed from the last iteration's messages by the lanes that own the first entry
        //      of a column, change places with the messages (X[j] = log-ratio of column j), then leave in whole rows ----
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = (LDPC_EDGE_PRIOR(r) + X[r * 64 + lane]) + X[paddr[r]];
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = scol_t[r * 64 + lane];
            if ((k0[r] >> lane) & 1ull) X[j] = msg[r];
        }
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk),
                            (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
#undef LDPC_EDGE_PRIOR
}

// ---- the same idea for heavier nodes: rows of weight <= 8 in EIGHT neighbouring lanes, columns of weight <= DC (<= 4) ----------
// Bivariate-bicycle codes (rows of 6, columns of 3: BB [[72,12,6]] ... [[144,12,12]]), small hypergraph products.  Differences to
// bp_edge_kernel:
//   * the butterfly over the other entries of a row has a third step across the two quads of the 8-lane group, the sign parity is a
//     BYTE parity of the lane mask (bp_edge_check8.h);
//   * a column has up to DC entries, so a lane reads ALL of them from the wave-private LDS array in column order and forms the
//     reference's sums with them; the lane's own k picks its bit_to_check (bp_edge_bit8.h).
struct Edge8Args {
    int32_t m, n, max_iter;
    double ms_scaling_factor;
    int64_t batch;
    const double *prior_s;     // [R * 64] prior of the slot's column; phantom: +inf          (general form)
    double prior_u;            // the one prior of every column                              (UNIFORM form)
    const uint16_t *cpos;      // [DC][R * 64] slot of the j-th entry of the slot's column, j < DC; beyond the column's weight: R * 64 (the +0.0
                               // slot); a phantom lane: R * 64 + 1 everywhere (a slot that holds +inf for good)
    const uint8_t *kind;       // [R * 64] 0 phantom, 1 + k for the k-th entry of its column
    const int32_t *scol;       // [R * 64] column of the slot; a phantom lane: R * 64 + 2 (the dummy slot)
    int32_t chunk;
    int32_t static_per, dyn_base, pool_per;  // (as EdgeArgs)
    const uint8_t *synd;
    uint8_t *decoding;
    double *llr;
    int32_t *iters;
    uint8_t *conv;
    unsigned long long *next;
    unsigned long long *clk;   // shader-clock probe (clock_probe_*, bp_device_common.h) or nullptr
};

namespace edge_detail {
// lane ^ 4 inside an 8-lane group: two DPP moves per dword, each writing only the banks (groups of 4 lanes) it is right for
__device__ __forceinline__ double xor4(double x) {
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x104, 0xf, 0x5, false);   // row_shl:4 -> banks 0, 2 (lanes 0-3, 8-11)
    lo = __builtin_amdgcn_update_dpp(lo, __double2loint(x), 0x114, 0xf, 0xa, false);      // row_shr:4 -> banks 1, 3
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x104, 0xf, 0x5, false);
    hi = __builtin_amdgcn_update_dpp(hi, __double2hiint(x), 0x114, 0xf, 0xa, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint64_t byte_parity_low(uint64_t x) {  // result in bit 0 of every byte; the other bits are garbage
    x ^= x >> 1;
    x ^= x >> 2;
    x ^= x >> 4;
    return x;
}
__device__ __forceinline__ uint64_t spread_byte(uint64_t low) {  // bit 0 of every byte -> all eight bits
    const uint32_t a = ((uint32_t)low & 0x01010101u) * 255u, b = ((uint32_t)(low >> 32) & 0x01010101u) * 255u;
    return ((uint64_t)b << 32) | a;
}
__device__ __forceinline__ double select_f64(double a, double b, uint64_t mask) {  // per lane: bit `lane` of mask ? b : a
    return __hiloint2double(select_by_mask(__double2hiint(a), __double2hiint(b), mask), select_by_mask(__double2loint(a), __double2loint(b), mask));
}
}  // namespace edge_detail

template <int R, int DC, bool UNIFORM>
__global__ void __launch_bounds__(64, UNIFORM ? 5 : 4) bp_edge8_kernel(const Edge8Args a) {
    using namespace edge_detail;
    typedef Edge8Args ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
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

    double prv[UNIFORM ? 1 : R], msg[R];
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
    const double pu = uniform_f64(a.prior_u);
#define LDPC_EDGE_PRIOR(r) (UNIFORM ? pu : prv[UNIFORM ? 0 : (r)])
    const double dbl_max = uniform_f64(DBL_MAX);
    if (lane == 0) { X[ZERO] = 0.0; X[ZERO + 1] = __builtin_inf(); }

    // Work: the static share, then chunks from the pooled work counters (work_pool_next, bp_device_common.h)
    int b0 = (int)blockIdx.x * LDPC_EDGE_ARG(static_per), b1 = b0 + LDPC_EDGE_ARG(static_per);
    int pool = (int)(blockIdx.x & (WORK_POOLS - 1));
    for (;;) {
      for (int b = b0; b < b1; ++b) {
#include "bp_edge_synd.h"  // sy[r], never
#pragma unroll
        for (int r = 0; r < R; ++r) msg[r] = phantom_lane[r] ? __builtin_inf() : LDPC_EDGE_PRIOR(r);  // initialise_log_domain_bp (bp.hpp:147-157)

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

        // ---- outputs: as bp_edge_kernel -- every lane of a column holds the column's log-ratio (the same bits) and parks it at X[column]
        //      (phantom lanes: at the dummy slot behind +inf), then whole rows leave ----
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double t = LDPC_EDGE_PRIOR(r);
#pragma unroll
            for (int j = 0; j < DC; ++j) t += X[caddr[r][j]];
            msg[r] = t;
        }
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
#pragma unroll
        for (int r = 0; r < R; ++r) X[scol_t[r * 64 + lane]] = msg[r];
#include "bp_edge_out_rows.h"
#include "bp_edge_out_status.h"
      }
        if (!work_pool_next(LDPC_EDGE_ARG(next), LDPC_EDGE_ARG(dyn_base), LDPC_EDGE_ARG(pool_per), LDPC_EDGE_ARG(chunk),
                            (int)LDPC_EDGE_ARG(batch), lane, pool, b0, b1)) break;
    }
    if (lane == 0) clock_probe_end(LDPC_EDGE_ARG(clk), clk_stamp);
#undef LDPC_EDGE_PRIOR
}
#undef LDPC_EDGE_ARG
