// bp_edge_gd_kernel.h -- bp_edge_gd_kernel, bp_edge8_gd_kernel: BP with guided decimation (BPGD) on the lane = edge min-sum kernels, all rounds of a syndrome in one launch
// Part of libldpc_hip.so: instantiated in tu_onchip_gd.hip, launched by host_onchip.h (decode_onchip_gd).
#pragma once

#include "bp_edge_kernel.h"

// ldpc_hip_bp_set_decimation on a code of the lane = edge families (the contract: tests/bpgd_util.py).  The check and bit
// passes are those of the general forms of bp_edge_kernel / bp_edge8_kernel (per-column prior, the clamp to DBL_MAX stays): the same
// fragments (bp_edge_kernel.h), with a prior register per lane and round as in bp_edge_rp_kernel.h -- inside a loop over the ROUNDS: one wavefront per
// syndrome, nothing leaves the chip between rounds.  A round is up to round_iters iterations; the iteration count runs on across the rounds
// (the scaling factor 0 takes alpha = 1 - 2^-it of the row's TOTAL it).  A round that ends without the syndrome reproduced, and is not the
// last, DECIMATES: the posteriors M of its last bit pass are formed from the check-to-bit messages that pass left in LDS (the outputs'
// expression), every lane keeps the best (|M|, column) of its own slots -- the column re-read from EdgeArgs::scol as the row-prior kernel
// does, rather than held in R more registers -- and a six-step butterfly over the wavefront finds the largest |M| and, among equal ones, the
// smallest column j*.  Every lane that holds an entry of j* then takes v = (M[j*] <= 0 ? -freeze_llr : +freeze_llr) for its prior AND its
// bit-to-check message, and marks the slot frozen; the other messages stay as they are.  frz: bit r = the lane's slot of round r is never
// chosen (again) -- set from the start where the prior is not finite (p = 0, 1 or NaN) and in the phantom lanes, which are known by their
// partner address (the +inf slot) as in bp_edge_rp_kernel: in bp_edge's tables a phantom lane carries column 0, a real column's, and it must
// neither win the reduction nor take v.  (bp_edge8's carry the dummy slot's number, R * 64 + 2, which no column has -- every column is used, so
// n <= nnz <= R * 64 -- and get the same bit all the same.)  A NaN posterior is never chosen.
// With nothing left to freeze the round still runs.  prv[], msg[] and frz are filled per SYNDROME from prior_s: a row pulled from the work
// pool starts from L0, not from its predecessor's frozen priors.
// iters = the iterations of all rounds run, conv = the syndrome was reproduced; outputs = the last bit pass (as bp_edge_kernel's).
// max_rounds = 1 is bp_edge_rp_kernel's decode with the handle's priors and max_iter = round_iters.
struct EdgeGdArgs {
    EdgeArgs e;                 // prior_s: L0 per slot; max_iter, prior_u: not read
    double freeze_llr;          // C > 0, finite or +inf
    int32_t round_iters, max_rounds;
};
struct Edge8GdArgs {
    Edge8Args e;
    double freeze_llr;
    int32_t round_iters, max_rounds;
};

typedef void (*EdgeGdKernel)(const EdgeGdArgs);
typedef void (*Edge8GdKernel)(const Edge8GdArgs);
// The instantiations live in tu_onchip_gd.hip; nullptr: no such instantiation (the ladders are those of plan_edge and plan_edge8).
EdgeGdKernel edge_gd_kernel(int rounds);
Edge8GdKernel edge8_gd_kernel(int rounds, int dc);

// Wavefronts per SIMD the instantiations are compiled for; the host sizes its grid by them (decode_onchip_gd).  What each instantiation
// compiles to is listed in DESIGN.md section 7e: the general form's four, except bp_edge_gd_kernel<15> and <16>, which at four spill 2 and 4
// VGPRs (12 and 20 bytes of scratch a lane) and get three.
__host__ __device__ constexpr int edge_gd_waves(int rounds) { return rounds <= 14 ? 4 : 3; }
__host__ __device__ constexpr int edge8_gd_waves(int, int) { return 4; }

namespace edge_detail {
// A lane's candidate for the column to freeze: key = |M| (-1: none), tag = 2 * column + (M <= 0) (INT_MAX: none).  Both lanes of a column hold
// the same pair.  `take`: the better of two -- the larger key, then the smaller tag, which is the smaller column.
struct GdPick { double key; int tag; };
__device__ __forceinline__ void gd_take(GdPick &p, double key, int tag, bool eligible) {
    if (eligible && (key > p.key || (key == p.key && tag < p.tag))) { p.key = key; p.tag = tag; }
}
__device__ __forceinline__ GdPick gd_wave_best(GdPick p) {
#pragma unroll
    for (int s = 1; s < LDPC_WAVE; s <<= 1) gd_take(p, __shfl_xor(p.key, s, LDPC_WAVE), __shfl_xor(p.tag, s, LDPC_WAVE), true);
    return p;  // (every lane holds the same pair)
}
}  // namespace edge_detail

// (LDPC_EDGE_ARG: bp_edge_kernel.h -- here the EdgeArgs / Edge8Args block is the member `e`)
#define LDPC_EDGE_ARG(field) LDPC_KERNARG(ARGS_T, e.field)
#define LDPC_EDGE_PRIOR(r) prv[r]  // the prior of the bit-pass fragments: a register per lane and round

template <int R>
__global__ void __launch_bounds__(64, edge_gd_waves(R)) bp_edge_gd_kernel(const EdgeGdArgs ga) {
    using namespace edge_detail;
    const EdgeArgs &a = ga.e;
    typedef EdgeGdArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    static_assert(R <= 32, "frz holds one bit per round");
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

    // per lane and round, for the whole kernel: partner address; per round: which lanes are first entries.  prv[r], frz: per SYNDROME, rewritten by a decimation
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
        // L0 again for THIS syndrome (whichever row the wavefront pulled): priors, initial messages (initialise_log_domain_bp, bp.hpp:147-157), frozen slots
        unsigned frz = 0;
        {
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                prv[r] = l0_t[r * 64 + lane];  // (phantom lanes: +inf)
                msg[r] = prv[r];
                if (paddr[r] == ZERO + 1 || !__builtin_isfinite(prv[r])) frz |= 1u << r;
            }
        }
#include "bp_edge_synd.h"  // sy[r], never

        const int round_iters = LDPC_KERNARG(ARGS_T, round_iters), max_rounds = LDPC_KERNARG(ARGS_T, max_rounds);
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
        int it = 0;
        bool unsat = true;
        for (int round = 0;; ++round) {
            const int stop = it + round_iters;
            do {
                ++it;
                const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
                // ---- check pass: msg[r] (bit_to_check) -> msg[r] (check_to_bit), stored at the slot ----
#include "bp_edge_check4.h"
                // ---- bit pass: the partner's message; log-ratio, decision, new bit_to_check ----
                uint64_t bad = 0;
#include "bp_edge_bit4.h"
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < stop);
            if (!unsat || round == max_rounds - 1) break;

            // ---- decimation: M of the round's last bit pass, by the column's FIRST entry (the outputs' expression); the largest |M|, then the smallest column ----
            GdPick pick = {-1.0, 0x7fffffff};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double mj = (prv[r] + X[r * 64 + lane]) + X[paddr[r]];
                const int j = scol_t[r * 64 + lane];
                gd_take(pick, __builtin_fabs(mj), (j << 1) | (mj <= 0.0 ? 1 : 0), ((k0[r] >> lane) & 1ull) && !((frz >> r) & 1u) && mj == mj);
            }
            pick = gd_wave_best(pick);
            const double v = (pick.tag & 1) ? -LDPC_KERNARG(ARGS_T, freeze_llr) : LDPC_KERNARG(ARGS_T, freeze_llr);
            const int jstar = pick.tag >> 1;  // (nothing left to freeze: no slot's column)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = scol_t[r * 64 + lane];
                if (j == jstar && !((frz >> r) & 1u)) {  // both entries of the column, wherever they sit; never a phantom lane (frozen from the start)
                    prv[r] = v;
                    msg[r] = v;
                    frz |= 1u << r;
                }
            }
        }

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
__global__ void __launch_bounds__(64, edge8_gd_waves(R, DC)) bp_edge8_gd_kernel(const Edge8GdArgs ga) {
    using namespace edge_detail;
    const Edge8Args &a = ga.e;
    typedef Edge8GdArgs ARGS_T;  // (cold fields: LDPC_KERNARG, bp_device_common.h)
    static_assert(DC >= 2 && DC <= 4, "columns of 2 .. 4 entries");
    static_assert(R <= 32, "frz holds one bit per round");
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
        // L0 again for THIS syndrome (see bp_edge_gd_kernel); phantom lanes: the first address is the +inf slot
        unsigned frz = 0;
        {
            const auto l0_t = global_ptr(LDPC_EDGE_ARG(prior_s));
#pragma unroll
            for (int r = 0; r < R; ++r) {
                prv[r] = l0_t[r * 64 + lane];  // (phantom lanes: +inf)
                msg[r] = prv[r];
                if (caddr[r][0] == ZERO + 1 || !__builtin_isfinite(prv[r])) frz |= 1u << r;
            }
        }
#include "bp_edge_synd.h"  // sy[r], never

        const int round_iters = LDPC_KERNARG(ARGS_T, round_iters), max_rounds = LDPC_KERNARG(ARGS_T, max_rounds);
        const auto scol_t = global_ptr(LDPC_EDGE_ARG(scol));
        int it = 0;
        bool unsat = true;
        for (int round = 0;; ++round) {
            const int stop = it + round_iters;
            do {
                ++it;
                const AlphaWords al = alpha_words(a.ms_scaling_factor, it);
                // ---- check pass (bp.hpp:220-273): minimum over the seven other lanes of the group, sign by the group's parity ----
#include "bp_edge_check8.h"
                // ---- bit pass (bp.hpp:276-318): the column's entries in order; log-ratio, decision, the lane's own bit_to_check ----
                uint64_t bad = 0;
#include "bp_edge_bit8.h"
                unsat = never || (bad & LOW) != 0;
            } while (unsat && it < stop);
            if (!unsat || round == max_rounds - 1) break;

            // ---- decimation (see bp_edge_gd_kernel): M is the forward sum's end value, the same in every lane of the column ----
            GdPick pick = {-1.0, 0x7fffffff};
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double mj = prv[r];
#pragma unroll
                for (int j = 0; j < DC; ++j) mj += X[caddr[r][j]];
                const int j = scol_t[r * 64 + lane];
                gd_take(pick, __builtin_fabs(mj), (j << 1) | (mj <= 0.0 ? 1 : 0), !((frz >> r) & 1u) && mj == mj);
            }
            pick = gd_wave_best(pick);
            const double v = (pick.tag & 1) ? -LDPC_KERNARG(ARGS_T, freeze_llr) : LDPC_KERNARG(ARGS_T, freeze_llr);
            const int jstar = pick.tag >> 1;  // (nothing left to freeze: no slot's column)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = scol_t[r * 64 + lane];
                if (j == jstar && !((frz >> r) & 1u)) {  // every entry of the column; never a phantom lane (frozen from the start)
                    prv[r] = v;
                    msg[r] = v;
                    frz |= 1u << r;
                }
            }
        }

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
