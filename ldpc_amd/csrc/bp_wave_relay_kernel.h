// bp_wave_relay_kernel.h -- bp_wave_relay_kernel: Relay-BP and memory min-sum on the lane = node kernel, a syndrome's messages and memory in LDS, all legs in one launch
// Part of libldpc_hip.so: instantiated in tu_onchip_wave_relay.hip, launched by host_onchip.h (decode_wave_relay).
#pragma once

#include "bp_wave_kernel.h"
#include "relay_common.h"

// ldpc_hip_bp_set_relay / ldpc_hip_bp_set_memory on a code beyond the lane = edge families (rows <= 16, columns <= 8, whatever fits LDS): the
// min-sum check and bit passes of bp_wave_kernel (bp_wave_kernel.h), operation by operation -- the structure-of-arrays M, the apos table, phantom
// entries, the reference's entry order and two sweeps; one wavefront, or (TEAM) the whole workgroup, per syndrome -- inside the leg loop of
// bp_edge_relay_kernel (bp_edge_relay_kernel.h).  One iteration -- alpha, both passes, the syndrome test, TEAM's flags -- is written once for this
// kernel and bp_wave_gd_kernel: the fragment bp_wave_ms_body.h, included below.  What differs from bp_wave_kernel:
//   the memory  Mprev[np], the posteriors of the last bit pass, lives beside the messages in the syndrome's private LDS region (always: there is no
//               llr_direct form).  The bit pass forms the prior of column j as mem_prior does (bp_spread_kernels.h): g == 0 ? a : a + g * Mprev[j],
//               the product rounded, then the sum.  The lane (team thread) that owns column j is the same in every bit pass: it reads the old value
//               and stores the new one, nobody else touches it.
//   a, gamma    of the leg from global memory in every bit pass (they stay in L2): WaveRelayArgs::ag_p, [legs][2][np], padded beyond n with a = 1.0
//               and gamma = 0 (wave_relay_table_kernel, host_onchip.h) -- a padding column forms the finite prior 1.0, decides 0 and never reaches
//               the weight or the outputs.  The priors L0, padded likewise, are WaveArgs::prior_g (always from global memory here).
//   the legs    leg 0 starts with messages and Mprev = L0; a later leg forms its messages from Mprev (real entries only: a row's phantom entries
//               keep +DBL_MAX, a column's the +0.0 slot) -- every real entry of M is rewritten before a bit pass reads one.  The iteration count
//               restarts at 1 in every leg.  A leg ends at the first bit pass whose decisions reproduce the syndrome (a syndrome byte > 1 never
//               does: the test compares bytes).  At a solution the weight is formed by ONE wavefront in relay_weight's order (TEAM: wavefront 0,
//               handed to the others through LDS -- a sum split over wavefronts would round differently); strictly lighter than the best so far:
//               the row's decoding and llr go to global memory, over an earlier solution's.  stop_after solutions end the row; a row without any
//               writes the last leg's last bit pass.  iters = the iterations of all legs run, conv = a solution was found.
// A memory decode is one leg of max_iter iterations with stop_after 1 (leg_iters == nullptr: every leg runs to WaveArgs::max_iter).
// Results are bit-identical to the per-pass kernels (host_stream.h: decode_relay, bp_spread_mem_*) and to the NumPy restatements
// (tests/relay_bp_util.py, tests/mem_bp_util.py).
struct WaveRelayArgs {
    WaveArgs w;                 // prior_g: always set; llr_direct, osd_*: not read
    const double *ag_p;         // [legs][2][np]: a, then gamma, of every column, per leg; beyond n: 1.0 and 0
    const int32_t *leg_iters;   // [legs], or nullptr: w.max_iter
    int32_t legs, stop_after;
};

typedef void (*WaveRelayKernel)(const WaveRelayArgs);
// The instantiations live in tu_onchip_wave_relay.hip: the six rungs of pick_wave (host_onchip.h), each with and without TEAM; nullptr: no such rung
WaveRelayKernel wave_relay_kernel(int dr, int dc, bool team);

// LDS bytes: the tables a workgroup shares / the private region of one syndrome (host and device agree through these)
__host__ __device__ inline size_t wave_relay_lds_shared(int mp, int np, int DR, int DC) {
    const size_t b = (size_t)DR * mp * 2 + (size_t)DC * np * 2 + (size_t)mp;
    return (b + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t wave_relay_lds_private(int mp, int np, int DR) { return wave_lds_private(mp, np, DR, true); }
// ... and what the host leaves free of the 160 KiB for the kernel's static __shared__ variables (plan_wave_relay; the kernel asserts that they fit)
constexpr size_t WAVE_RELAY_LDS_STATIC = 64;

template <int DR, int DC, bool TEAM>
__global__ void __launch_bounds__(64 * wave_ms_waves(DR, DC, TEAM)) bp_wave_relay_kernel(const WaveRelayArgs ra) {
    const WaveArgs &a = ra.w;
    constexpr int U = wave_ms_nodes_per_lane(DR, DC);
    constexpr int UC = TEAM ? 1 : U;
    extern __shared__ __attribute__((aligned(16))) unsigned char wv_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tl = TEAM ? tid : lane, TS = TEAM ? T : 64;    // this thread within the team that shares a syndrome, the team's size
    const int wt = TEAM ? wave : 0, W = TEAM ? T >> 6 : 1;   // this wavefront within the team, wavefronts of a team
    __shared__ int team_unsat[2];
    __shared__ long long team_b;
    __shared__ double team_w;
    __shared__ unsigned long long clk_stamp[2];
    static_assert(sizeof(team_unsat) + sizeof(team_b) + sizeof(team_w) + sizeof(clk_stamp) <= WAVE_RELAY_LDS_STATIC, "the host plans the dynamic LDS with this much left for the static part");
    if (threadIdx.x == 0) clock_probe_begin(clk_stamp);
    auto team_sync = [&]() { if (TEAM) __syncthreads(); else __builtin_amdgcn_wave_barrier(); };
    const int m = a.m, n = a.n, mp = a.mp, np = a.np, rm = DR * mp, cn = DC * np;
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) uint16_t lds_u16;
    typedef __attribute__((address_space(3))) uint64_t lds_u64;
    lds_u8 *base = (lds_u8 *)wv_lds;
    // shared, read-only after the barrier below: [col][apos][rdeg]
    lds_u16 *col = (lds_u16 *)base;
    lds_u16 *apos = col + rm;
    lds_u8 *rdeg = (lds_u8 *)(apos + cn);
    for (int q = tid; q < mp; q += T) rdeg[q] = a.rdeg[q];
    for (int q = tid; q < rm; q += T) col[q] = a.col[q];
    for (int q = tid; q < cn; q += T) apos[q] = a.apos[q];
    __syncthreads();

    // private to a syndrome: [M DR*mp][dummy][+0.0][Mprev np][hard decisions np/64 + 1 words, the last one zero][syndrome bytes mp]
    lds_u8 *mine = base + a.lds_shared + (TEAM ? 0 : wave) * a.lds_per_wave;
    lds_f64 *M = (lds_f64 *)mine;
    lds_f64 *L = M + rm + 2;
    volatile lds_u64 *hardw = (volatile lds_u64 *)(L + np);
    volatile lds_u8 *sy = (volatile lds_u8 *)(hardw + np / 64 + 1);
    const int DUMMY = rm, ZERO = rm + 1;
    if (tl == 0) { M[ZERO] = 0.0; hardw[np / 64] = 0; team_unsat[0] = 0; team_unsat[1] = 0; }
    for (int q = tl; q < mp; q += TS) sy[q] = 0;
    team_sync();

    const int legs = ra.legs, stop_after = ra.stop_after;
    int pool = (int)((blockIdx.x * (T / 64) + wave) & (WORK_POOLS - 1));  // work_pool_next (bp_device_common.h)
    bool first_turn = true;
    for (;;) {
        int64_t b;
        if (TEAM && a.next == nullptr) {  // no more syndromes than teams: team g takes syndrome g (bp_wave_kernel)
            b = first_turn ? (int64_t)blockIdx.x : a.batch;
            first_turn = false;
        } else if (TEAM) {
            if (tid == 0) team_b = (long long)atomicAdd(a.next, 1ull);
            __syncthreads();
            b = team_b;
        } else {
            int b0 = 0, b1 = 0;
            b = work_pool_next(a.next, 0, a.pool_per, 1, (int)a.batch, lane, pool, b0, b1) ? (int64_t)b0 : a.batch;
        }
        if (b >= a.batch) break;
        // this syndrome's bytes; leg 0: messages and Mprev = L0 (initialise_log_domain_bp, bp.hpp:147-157); phantom entries get +DBL_MAX (prior_g[np])
        for (int i = tl; i < m; i += TS) sy[i] = a.synd[b * m + i];
        for (int q = tl; q < rm; q += TS) M[q] = a.prior_g[col[q]];
        for (int q = tl; q < np; q += TS) L[q] = a.prior_g[q];
        if (TEAM && tid == 0) { team_unsat[0] = 0; team_unsat[1] = 0; }  // (a syndrome that ran out of iterations leaves its last flag raised)
        team_sync();

        // the row's state: reset with every syndrome pulled
        double best = __builtin_inf();
        int nsol = 0, total = 0;
        for (int leg = 0; leg < legs; ++leg) {
            const double *a_t = ra.ag_p + (size_t)leg * 2 * (size_t)np;  // the leg's tables: a, then gamma
            const double *g_t = a_t + np;
            const int leg_iters = ra.leg_iters ? ra.leg_iters[leg] : a.max_iter;
            const bool last = leg == legs - 1;
            if (leg > 0) {  // the initial messages of a later leg, from Mprev; a row's phantom entries keep their +DBL_MAX
                for (int q = tl; q < rm; q += TS) {
                    const int cj = col[q];
                    if (cj < np) {
                        const double as = a_t[cj], gs = g_t[cj];
                        M[q] = gs == 0.0 ? as : as + gs * L[cj];
                    }
                }
                team_sync();
            }

            int it = 0;
            bool unsat_any = true;
            // one iteration: bp_wave_ms_body.h.  The prior of column j as mem_prior forms it (a select: a + 0 * inf would be NaN); the flags by all legs' iterations
#define WAVE_MS_SET_PRIOR(pr, j, word) { const double as = a_t[j], gs = g_t[j], prev = L[j]; pr = gs == 0.0 ? as : as + gs * prev; }
#define WAVE_MS_ITERATIONS (total + it)
            do {
#include "bp_wave_ms_body.h"
            } while (unsat_any && it < leg_iters);
            total += it;

            // ---- the leg's end: a solution, or the last leg of a row without one.  unsat_any, nsol and best are the same in every thread of the team ----
            if (!unsat_any || (last && nsol == 0)) {
                bool take = unsat_any;
                if (!unsat_any) {
                    double w = 0.0;
                    if (!TEAM || wave == 0) w = relay_weight(a.llr0, n, lane, [&](int j) { return ((hardw[j >> 6] >> (j & 63)) & 1ull) != 0; });
                    if (TEAM) {
                        if (tid == 0) team_w = w;
                        __syncthreads();
                        w = team_w;
                    }
                    ++nsol;
                    if (w < best) { best = w; take = true; }
                }
                if (take)
                    for (int j = tl; j < n; j += TS) {
                        a.decoding[b * n + j] = (uint8_t)((hardw[j >> 6] >> (j & 63)) & 1ull);
                        if (a.llr) a.llr[b * n + j] = L[j];
                    }
            }
            if (nsol == stop_after) break;
        }
        if (tl == 0) {
            if (a.iters) a.iters[b] = total;
            if (a.conv) a.conv[b] = nsol > 0 ? 1 : 0;
        }
        team_sync();
    }
    if (threadIdx.x == 0) clock_probe_end(a.clk, clk_stamp);
}
