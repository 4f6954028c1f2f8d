// bp_wave_gd_kernel.h -- bp_wave_gd_kernel: BP with guided decimation (BPGD) on the lane = node kernel, a syndrome's messages, posteriors and frozen columns in LDS, all rounds in one launch
// Part of libldpc_hip.so: instantiated in tu_onchip_wave_gd.hip, launched by host_onchip.h (decode_wave_gd).
#pragma once

#include "bp_wave_kernel.h"
#include "bp_edge_gd_kernel.h"  // (GdPick, gd_take, gd_wave_best: the lane = edge decimation kernels' candidate and its butterfly)

// ldpc_hip_bp_set_decimation with ldpc_hip_bp_set_decimation_lane_node on a code beyond the lane = edge families (rows <= 16, columns <= 8,
// whatever fits LDS; the contract: tests/bpgd_util.py).  The skeleton is bp_wave_relay_kernel's (bp_wave_relay_kernel.h),
// operation by operation: the min-sum check pass, bit pass and syndrome test of bp_wave_kernel, the structure-of-arrays M, the apos table,
// phantom entries, the DUMMY / ZERO slots, one wavefront or (TEAM) the whole workgroup per syndrome, work_pool_next or the static team share,
// the clock probe.  One iteration is the same text in both: the fragment bp_wave_ms_body.h, included below.  What differs:
//   the rounds  in place of the legs: a round is up to round_iters iterations (stop = it + round_iters) and `it` is never reset -- the scaling
//               factor 0 takes alpha = 1 - 2^-it of the row's TOTAL, and TEAM's two flags are indexed by that total.
//   the prior   of column j in the bit pass is D[j] ? (S[j] ? -C : +C) : prior_g[j]: D (decimated) and S (the frozen sign) are two bit masks
//               of np / 64 + 1 words in the syndrome's private LDS region beside the hard decisions, cleared with every syndrome pulled -- a
//               row from the work pool starts from L0, not from its predecessor's frozen columns.  The word of a lane's column is the same for
//               the whole wavefront (one broadcast read); there is no a / gamma table and no memory term.  L[np] stays: the posteriors of the
//               last bit pass are the outputs and what a decimation looks at.
//   decimation  after a round's last iteration, unsolved and not the last round: the candidates are the columns j < n with D[j] clear, a
//               finite prior_g[j] and L[j] not NaN; the key is |L[j]|, the largest wins, among equal ones the smallest j.  Every thread walks
//               its own columns ascending and keeps a strictly larger key; gd_wave_best reduces a wavefront; TEAM: every wavefront's winner
//               goes through a static LDS array and every thread reduces that array in the same order.  No candidate: (-1, INT_MAX), nothing
//               changes and the round still runs.  The padding columns (j >= n) are never looked at.
//   freezing    v = (L[j*] <= 0) ? -C : +C; the D and S bits of j* are set and every real entry of column j* in M -- bit-to-check messages
//               after a bit pass -- becomes v.  L is not touched.
// iters = the iterations of all rounds run, conv = the syndrome was reproduced; the outputs are the last bit pass's, written once.
// max_rounds = 1 is bp_wave_kernel's min-sum decode with max_iter = round_iters.
struct WaveGdArgs {
    WaveArgs w;                 // prior_g: always set; max_iter, llr_direct, osd_*: not read
    double freeze_llr;          // C > 0, finite or +inf
    int32_t round_iters, max_rounds;
};

typedef void (*WaveGdKernel)(const WaveGdArgs);
// The instantiations live in tu_onchip_wave_gd.hip: the six rungs of pick_wave (host_onchip.h), each with and without TEAM; nullptr: no such rung
WaveGdKernel wave_gd_kernel(int dr, int dc, bool team);

// LDS bytes of the private region of one syndrome (host and device agree through this; the shared tables are bp_wave_relay_kernel's:
// wave_relay_lds_shared): bp_wave_kernel's with the posterior copy, and the two masks D and S behind the hard decisions.
__host__ __device__ inline size_t wave_gd_lds_private(int mp, int np, int DR) {  // [M + 2][L][hardw, D, S][syndrome bytes]
    const size_t b = ((size_t)DR * mp + 2) * 8 + (size_t)np * 8 + 3 * (size_t)(np / 64 + 1) * 8 + (size_t)mp;
    return (b + 15) & ~(size_t)15;
}

// ... and what the host leaves free of the 160 KiB for the kernel's static __shared__ variables (plan_wave_gd; ldpc_amd.bpgd_decoder.lane_node_takes
// restates it): the relay kernel's 40 bytes and the teams' winners, 16 x (8 + 4) -- 224 bytes in the team forms.  The kernel asserts that they fit.
constexpr size_t WAVE_GD_LDS_STATIC = 256;

template <int DR, int DC, bool TEAM>
__global__ void __launch_bounds__(64 * wave_ms_waves(DR, DC, TEAM)) bp_wave_gd_kernel(const WaveGdArgs ga) {
    using edge_detail::GdPick;
    using edge_detail::gd_take;
    using edge_detail::gd_wave_best;
    const WaveArgs &a = ga.w;
    constexpr int U = wave_ms_nodes_per_lane(DR, DC);
    constexpr int UC = TEAM ? 1 : U;
    constexpr int MAXW = 16;  // (wave_ms_waves never gives a team more)
    static_assert(wave_ms_waves(DR, DC, true) <= MAXW, "team_key / team_tag hold one winner per wavefront");
    extern __shared__ __attribute__((aligned(16))) unsigned char wv_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tl = TEAM ? tid : lane, TS = TEAM ? T : 64;    // this thread within the team that shares a syndrome, the team's size
    const int wt = TEAM ? wave : 0, W = TEAM ? T >> 6 : 1;   // this wavefront within the team, wavefronts of a team
    __shared__ int team_unsat[2];
    __shared__ long long team_b;
    __shared__ double team_key[MAXW];
    __shared__ int team_tag[MAXW];
    __shared__ unsigned long long clk_stamp[2];
    static_assert(sizeof(team_unsat) + sizeof(team_b) + sizeof(team_key) + sizeof(team_tag) + sizeof(clk_stamp) <= WAVE_GD_LDS_STATIC,
                  "the host plans the dynamic LDS with this much left for the static part");
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

    // private to a syndrome: [M DR*mp][dummy][+0.0][L np][hard decisions np/64 + 1 words, the last one zero][D np/64 + 1][S np/64 + 1][syndrome bytes mp]
    const int nw = np / 64 + 1;
    lds_u8 *mine = base + a.lds_shared + (TEAM ? 0 : wave) * a.lds_per_wave;
    lds_f64 *M = (lds_f64 *)mine;
    lds_f64 *L = M + rm + 2;
    volatile lds_u64 *hardw = (volatile lds_u64 *)(L + np);
    volatile lds_u64 *Dm = hardw + nw;
    volatile lds_u64 *Sm = Dm + nw;
    volatile lds_u8 *sy = (volatile lds_u8 *)(Sm + nw);
    const int DUMMY = rm, ZERO = rm + 1;
    if (tl == 0) { M[ZERO] = 0.0; hardw[np / 64] = 0; team_unsat[0] = 0; team_unsat[1] = 0; }
    for (int q = tl; q < mp; q += TS) sy[q] = 0;
    team_sync();

    const int round_iters = ga.round_iters, max_rounds = ga.max_rounds;
    const double C = ga.freeze_llr;
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
        // this syndrome's bytes; messages and L = L0 (initialise_log_domain_bp, bp.hpp:147-157); phantom entries get +DBL_MAX (prior_g[np]); nothing frozen
        for (int i = tl; i < m; i += TS) sy[i] = a.synd[b * m + i];
        for (int q = tl; q < rm; q += TS) M[q] = a.prior_g[col[q]];
        for (int q = tl; q < np; q += TS) L[q] = a.prior_g[q];
        for (int q = tl; q < nw; q += TS) { Dm[q] = 0; Sm[q] = 0; }
        if (TEAM && tid == 0) { team_unsat[0] = 0; team_unsat[1] = 0; }  // (a syndrome that ran out of iterations leaves its last flag raised)
        team_sync();

        int it = 0;  // the row's total: never reset between rounds
        bool unsat_any = true;
        for (int round = 0;; ++round) {
            const int stop = it + round_iters;
            // one iteration: bp_wave_ms_body.h.  A frozen column's prior is +-C (the wavefront's 64 columns: one word of each mask); the flags by the row's total
#define WAVE_MS_SET_PRIOR(pr, j, word) { const uint64_t dw = Dm[word], sw = Sm[word]; const double l0 = a.prior_g[j]; pr = ((dw >> lane) & 1ull) ? (((sw >> lane) & 1ull) ? -C : C) : l0; }
#define WAVE_MS_ITERATIONS it
            do {
#include "bp_wave_ms_body.h"
            } while (unsat_any && it < stop);
            if (!unsat_any || round == max_rounds - 1) break;  // (unsat_any is the same in every thread of the team)

            // ---- decimation: the largest |L| among the columns not frozen, with a finite prior and a posterior that is no NaN; then the smallest column ----
            GdPick pick = {-1.0, 0x7fffffff};
            for (int j = tl; j < n; j += TS) {
                const double lj = L[j];
                const bool open = !((Dm[j >> 6] >> (j & 63)) & 1ull) && __builtin_isfinite(a.prior_g[j]) && lj == lj;
                if (open && __builtin_fabs(lj) > pick.key) { pick.key = __builtin_fabs(lj); pick.tag = j; }  // ascending: a strictly larger key only
            }
            pick = gd_wave_best(pick);
            if (TEAM) {  // every wavefront's winner through LDS; every thread reduces them in the same order
                if (lane == 0) { team_key[wave] = pick.key; team_tag[wave] = pick.tag; }
                __syncthreads();
                pick = GdPick{-1.0, 0x7fffffff};
                for (int w = 0; w < W; ++w) gd_take(pick, team_key[w], team_tag[w], true);
            }
            if (pick.tag != 0x7fffffff) {  // (nothing left to freeze: nothing changes)
                const int jstar = pick.tag;
                const bool neg = L[jstar] <= 0;
                const double v = neg ? -C : C;
                if (tl == 0) {
                    const uint64_t bit = 1ull << (jstar & 63);
                    Dm[jstar >> 6] = Dm[jstar >> 6] | bit;
                    if (neg) Sm[jstar >> 6] = Sm[jstar >> 6] | bit;
                }
                if (tl < DC) {  // the column's bit-to-check messages; a phantom entry's +0.0 slot stays
                    const int pos = apos[tl * np + jstar];
                    if (pos != ZERO) M[pos] = v;
                }
            }
            team_sync();
        }

        // ---- outputs: this bit pass (converged, iters = it) or the last one (iters = max_rounds * round_iters), written once ----
        for (int j = tl; j < n; j += TS) {
            a.decoding[b * n + j] = (uint8_t)((hardw[j >> 6] >> (j & 63)) & 1ull);
            if (a.llr) a.llr[b * n + j] = L[j];
        }
        if (tl == 0) {
            if (a.iters) a.iters[b] = it;
            if (a.conv) a.conv[b] = unsat_any ? 0 : 1;
        }
        team_sync();
    }
    if (threadIdx.x == 0) clock_probe_end(a.clk, clk_stamp);
}
