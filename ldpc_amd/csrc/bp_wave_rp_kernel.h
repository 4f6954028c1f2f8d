// bp_wave_rp_kernel.h -- bp_wave_rp_kernel: min-sum with row priors on the lane = node kernel, every syndrome decoded with its own priors, its messages and posteriors in LDS
// Part of libldpc_hip.so: instantiated in tu_onchip_wave_rp.hip, launched by host_onchip.h (decode_wave_rp).
#pragma once

#include "bp_wave_kernel.h"

// ldpc_hip_*_decode_batch_priors, min-sum, on a code beyond the lane = edge families (rows <= 16, columns <= 8, whatever fits LDS; DESIGN.md
// section 4).  The skeleton is bp_wave_relay_kernel's and bp_wave_gd_kernel's, operation by operation: the min-sum check pass, bit pass and syndrome
// test of bp_wave_kernel, the structure-of-arrays M, the apos table, phantom entries, the DUMMY / ZERO slots, one wavefront or (TEAM) the whole
// workgroup per syndrome, work_pool_next or the static team share, the clock probe.  One iteration is the same text in all three: the fragment
// bp_wave_ms_body.h, included below.  What differs from bp_wave_kernel's min-sum form with WaveArgs::prior_g:
//   the priors  are those of the SYNDROME: row b of WaveRpArgs::rowp, [batch][np + 2] log-ratios padded as wave_prior_pad_kernel pads the shared
//               ones (1.0 for the columns n .. np - 1, DBL_MAX at np: a row's phantom entries; wave_rp_prior_kernel, host_onchip.h).  b is the
//               syndrome index pulled from the work pool -- or blockIdx.x where the teams are static -- never the wavefront's or the team's own
//               number, and the row's offset b (np + 2) is formed in 64 bits.  The bit pass reads its column's prior from that row in every
//               iteration (8 (np + 2) bytes a syndrome: they stay in L2), as the lean form of bp_wave_kernel reads the shared ones.
//   the posteriors  L[np] are always in LDS (the fragment stores them in every bit pass); there is no llr_direct form.
// iters, conv and the outputs of the last bit pass are bp_wave_kernel's.  No OSD hand-over: after a row-prior decode bposd_device lists the unsolved
// rows itself (host_osd.h), as after the relay and decimation kernels.
struct WaveRpArgs {
    WaveArgs w;           // prior_g, llr0, llr_direct, osd_*: not read
    const double *rowp;   // [batch][np + 2]: every syndrome's own priors, padded
};

typedef void (*WaveRpKernel)(const WaveRpArgs);
// The instantiations live in tu_onchip_wave_rp.hip: the six rungs of pick_wave (host_onchip.h), each with and without TEAM; nullptr: no such rung
WaveRpKernel wave_rp_kernel(int dr, int dc, bool team);

// LDS bytes: the tables a workgroup shares / the private region of one syndrome (host and device agree through these): [col][apos][rdeg] and
// bp_wave_kernel's region with the posterior copy
__host__ __device__ inline size_t wave_rp_lds_shared(int mp, int np, int DR, int DC) {
    const size_t b = (size_t)DR * mp * 2 + (size_t)DC * np * 2 + (size_t)mp;
    return (b + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t wave_rp_lds_private(int mp, int np, int DR) { return wave_lds_private(mp, np, DR, true); }
// ... and what the host leaves free of the 160 KiB for the kernel's static __shared__ variables (plan_wave_rp; the kernel asserts that they fit)
constexpr size_t WAVE_RP_LDS_STATIC = 64;

template <int DR, int DC, bool TEAM>
__global__ void __launch_bounds__(64 * wave_ms_waves(DR, DC, TEAM)) bp_wave_rp_kernel(const WaveRpArgs ra) {
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
    __shared__ unsigned long long clk_stamp[2];
    static_assert(sizeof(team_unsat) + sizeof(team_b) + sizeof(clk_stamp) <= WAVE_RP_LDS_STATIC, "the host plans the dynamic LDS with this much left for the static part");
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

    // private to a syndrome: [M DR*mp][dummy][+0.0][L np][hard decisions np/64 + 1 words, the last one zero][syndrome bytes mp]
    lds_u8 *mine = base + a.lds_shared + (TEAM ? 0 : wave) * a.lds_per_wave;
    lds_f64 *M = (lds_f64 *)mine;
    lds_f64 *L = M + rm + 2;
    volatile lds_u64 *hardw = (volatile lds_u64 *)(L + np);
    volatile lds_u8 *sy = (volatile lds_u8 *)(hardw + np / 64 + 1);
    const int DUMMY = rm, ZERO = rm + 1;
    if (tl == 0) { M[ZERO] = 0.0; hardw[np / 64] = 0; team_unsat[0] = 0; team_unsat[1] = 0; }
    for (int q = tl; q < mp; q += TS) sy[q] = 0;
    team_sync();

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
        // this syndrome's bytes and ITS priors: row b of rowp (64-bit offset); messages = L0 (initialise_log_domain_bp, bp.hpp:147-157); phantom entries get +DBL_MAX (row[np])
        const double *const prior_b = ra.rowp + (size_t)b * (size_t)(np + 2);
        for (int i = tl; i < m; i += TS) sy[i] = a.synd[b * m + i];
        for (int q = tl; q < rm; q += TS) M[q] = prior_b[col[q]];
        if (TEAM && tid == 0) { team_unsat[0] = 0; team_unsat[1] = 0; }  // (a syndrome that ran out of iterations leaves its last flag raised)
        team_sync();

        int it = 0;
        bool unsat_any = true;
        // one iteration: bp_wave_ms_body.h.  The prior of column j is the syndrome's own
#define WAVE_MS_SET_PRIOR(pr, j, word) { pr = prior_b[j]; }
#define WAVE_MS_ITERATIONS it
        do {
#include "bp_wave_ms_body.h"
        } while (unsat_any && it < a.max_iter);

        // ---- outputs: this bit pass (converged) or the last one, written once ----
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
