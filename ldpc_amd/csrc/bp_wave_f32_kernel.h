// bp_wave_f32_kernel.h -- bp_wave_f32_kernel: the lane = node min-sum kernel of bp_wave_kernel.h with FP32 messages, a syndrome's messages in LDS
// Part of libldpc_hip.so: instantiated in tu_onchip_wave_f32.hip, launched by host_onchip.h (decode_wave_f32).
//
// The float32 message mode (ldpc_hip_bp_set_message_dtype) on the codes beyond both lane = edge ladders -- rows <= 16,
// columns <= 8, a syndrome's state within LDS: hypergraph products, BB288, detector error models -- with ldpc_hip_bp_set_f32_lane_node on (opt-in).
// It is the min-sum half of bp_wave_kernel restated for a 32-bit value; the FP64 template is not touched and not parametrised by the type.
//
// Reused as they are: the u16 column and position tables (ensure_wave_tables: positions count ELEMENTS of M, so they serve either type), the
// layout of M -- entry k of row i at M[k * mp + i]; a row's phantom entries hold the neutral element for good (here FLT_MAX), their stores
// redirected to the dummy slot; a column's phantom entries point at the slot that holds +0.0f -- the nodes per lane in flight
// (wave_ms_nodes_per_lane), the TEAM form (workgroup barriers between the passes, the two alternating team_unsat flags, team_b), how work is
// drawn (static teams when next == nullptr, else the first counter for teams and work_pool_next for lone wavefronts) and the clock probe.
//
// Arithmetic: that of bp_f32_kernels.h, of bp_edge_f32_kernel.h and of tests/f32_util.py: min_sum_restatement(..., np.float32), which binds --
// the three float32 routes give the same bits.
//   priors       the handle's FP64 log((1 - p) / p) rounded ONCE to FP32 (v_cvt_f32_f64), read ALWAYS from the padded device array
//                WaveF32Args::prior_g: [np + 2] floats, 1.0f beyond n, FLT_MAX at np (wave_f32_prior_kernel, before every launch, in this decode's
//                element type).  No LDS copy: bp_wave_relay_kernel makes the same choice, and it removes one form.
//   check pass   the reference's two sweeps with its comparisons (`a < temp`, which decide NaNs as the restatement does); the minimum starts from
//                FLT_MAX, so an infinite |bit_to_check| never enters it; sign = parity(syndrome byte + #{entries <= 0}) + own;
//                message = magnitude * (sgn ? -alpha : alpha) in ONE multiply; alpha is formed in FP64 (1 - 2^-it where the factor is 0) and
//                rounded once.
//   bit pass     forward partial sums from the prior, backward partial sums from +0.0f, ONE FP32 addition each, the reference's operand order;
//                posterior = the forward sum, decision = posterior <= 0.
// Neutral elements change no bit, as in FP64: min(x, FLT_MAX) = x for every x the minimum admits, and x + 0.0f = x unless x is -0.0f -- the FP32
// prior is never -0.0f (bp_edge_f32_kernel.h says why) and a sum is -0.0f only if both terms are.
// Nothing is contracted (the pragma below, and -ffp-contract=off in the Makefile); FP32 denormals are kept (the unit is built like every unit,
// without -fgpu-flush-denormals-to-zero: its kernel descriptors say FP32 denormal mode 3).
// A syndrome byte > 1 never converges: the test compares the byte.  Output freezing, `iters` and `conv` are bp_wave_kernel's.
// Log-ratios leave as FP64, each the FP32 posterior widened exactly (v_cvt_f64_f32) by the lane that holds it: no transpose launch.  Two runtime
// forms when they are asked for, as in FP64: a copy of the posteriors in LDS (np * 4 bytes), stored once at the end, or llr_direct -- every bit pass
// stores them widened to HBM and the last pass's values stay.
// No OSD hook: bposd_device lists the unsolved rows itself, as after the lane = edge FP32 kernels and the relay kernels.
#pragma once

#include "bp_wave_kernel.h"

#pragma clang fp contract(off)

struct WaveF32Args {
    int32_t m, n, mp, np, max_iter;
    int32_t llr_direct;          // 1: every bit pass stores its log-ratios, widened, straight to a.llr (no LDS copy)
    double ms_scaling_factor;
    int64_t batch;
    const uint8_t *rdeg;         // [mp] row degrees (0 for padding rows)
    const uint16_t *col;         // [DR * mp] column of the k-th entry of row i at [k * mp + i]; phantom: np
    const uint16_t *apos;        // [DC * np] position in M of the k-th entry of column j at [k * np + j]; phantom: DR * mp + 1
    const double *llr0;          // (not read: the launch helper sets it for every lane = node kernel)
    const float *prior_g;        // [np + 2] the priors rounded to FP32; 1.0f beyond n, FLT_MAX at np (a row's phantom entries)
    const uint8_t *synd;         // [batch][m]
    uint8_t *decoding;           // [batch][n]
    double *llr;                 // [batch][n] or nullptr: FP32 posteriors, widened
    int32_t *iters;              // [batch] or nullptr
    uint8_t *conv;               // [batch] or nullptr
    unsigned long long *next;    // WORK_POOLS work counters (work_pool_next; zeroed before launch), or nullptr: static teams
    int32_t pool_per;            // syndromes per pool
    int32_t lds_shared, lds_per_wave;  // bytes
    unsigned long long *clk;     // shader-clock probe or nullptr
};

typedef void (*WaveF32Kernel)(const WaveF32Args);
typedef void (*WaveF32PriorKernel)(const double *, int, int, float *);
// The instantiations live in tu_onchip_wave_f32.hip: the six rungs of LDPC_WAVE_LADDER (host_onchip.h), each with and without TEAM; nullptr: no such rung
WaveF32Kernel wave_f32_kernel(int dr, int dc, bool team);
// ... and the kernel that writes WaveF32Args::prior_g (llr0 [n], n, np, out [np + 2])
WaveF32PriorKernel wave_f32_prior_kernel();

// LDS bytes: the tables a workgroup shares / the private region of one syndrome (host and device agree through these)
__host__ __device__ inline size_t wave_f32_lds_shared(int mp, int np, int DR, int DC) {
    const size_t b = (size_t)DR * mp * 2 + (size_t)DC * np * 2 + (size_t)mp;
    return (b + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t wave_f32_lds_private(int mp, int np, int DR, bool want_llr) {
    const size_t b = ((size_t)DR * mp + 2) * 4 + (want_llr ? (size_t)np * 4 : 0) + (size_t)(np / 64 + 1) * 8 + (size_t)mp;
    return (b + 15) & ~(size_t)15;
}
// ... and what the host leaves free of the 160 KiB for the kernel's static __shared__ variables (plan_wave_f32; the kernel asserts that they fit)
constexpr size_t WAVE_F32_LDS_STATIC = 64;
// Wavefronts per workgroup the instantiations are compiled for (__launch_bounds__) -- the host launches no more (plan_wave_f32).  Sixteen for all
// twelve: none spills a VGPR at 128 registers (DESIGN.md section 7a has the table), so nothing is lowered the way wave_ms_waves lowers two FP64 forms.
__host__ __device__ constexpr int wave_f32_waves(int, int, bool) { return 16; }

template <int DR, int DC, bool TEAM>
__global__ void __launch_bounds__(64 * wave_f32_waves(DR, DC, TEAM)) bp_wave_f32_kernel(const WaveF32Args a) {
    constexpr int U = wave_ms_nodes_per_lane(DR, DC);  // nodes per lane in flight, as bp_wave_kernel
    constexpr int UC = TEAM ? 1 : U;                   // (a team: one row per lane in the check pass, so that twice as many wavefronts take part)
    extern __shared__ __attribute__((aligned(16))) unsigned char wv_lds[];
    const int tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tl = TEAM ? tid : lane, TS = TEAM ? T : 64;    // this thread within the team that shares a syndrome, the team's size
    const int wt = TEAM ? wave : 0, W = TEAM ? T >> 6 : 1;   // this wavefront within the team, wavefronts of a team
    __shared__ int team_unsat[2];
    __shared__ long long team_b;
    __shared__ unsigned long long clk_stamp[2];
    static_assert(sizeof(team_unsat) + sizeof(team_b) + sizeof(clk_stamp) <= WAVE_F32_LDS_STATIC, "the host plans the dynamic LDS with this much left for the static part");
    if (threadIdx.x == 0) clock_probe_begin(clk_stamp);
    auto team_sync = [&]() { if (TEAM) __syncthreads(); else __builtin_amdgcn_wave_barrier(); };
    const int m = a.m, n = a.n, mp = a.mp, np = a.np, rm = DR * mp, cn = DC * np;
    const bool want_llr = a.llr != nullptr && !a.llr_direct, llr_direct = a.llr != nullptr && a.llr_direct;
    // Every LDS pointer is typed in the LDS address space from the start (bp_wave_kernel.h says why)
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    typedef __attribute__((address_space(3))) float lds_f32;
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

    // private to a syndrome: [M DR*mp][dummy][+0.0f][posteriors np, if copied][hard decisions np/64 + 1 words, the last one zero][syndrome bytes mp]
    lds_u8 *mine = base + a.lds_shared + (TEAM ? 0 : wave) * a.lds_per_wave;
    lds_f32 *M = (lds_f32 *)mine;
    lds_f32 *L = M + rm + 2;
    volatile lds_u64 *hardw = (volatile lds_u64 *)(L + (want_llr ? np : 0));
    volatile lds_u8 *sy = (volatile lds_u8 *)(hardw + np / 64 + 1);
    const int DUMMY = rm, ZERO = rm + 1;
    if (tl == 0) { M[ZERO] = 0.0f; hardw[np / 64] = 0; team_unsat[0] = 0; team_unsat[1] = 0; }
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
        // initialise_log_domain_bp (bp.hpp:147-157) + this syndrome's bytes; phantom entries get FLT_MAX (prior_g[np])
        for (int i = tl; i < m; i += TS) sy[i] = a.synd[b * m + i];
        for (int q = tl; q < rm; q += TS) M[q] = a.prior_g[col[q]];
        if (TEAM && tid == 0) { team_unsat[0] = 0; team_unsat[1] = 0; }  // (a syndrome that ran out of iterations leaves its last flag raised)
        team_sync();

        int it = 0;
        bool unsat_any = true;
        do {
            ++it;
            const float alpha = (float)((a.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.ms_scaling_factor);  // FP64, then one rounding
            // ---- check pass (bp.hpp:201-273), in place, UC rows per lane in flight: loads, arithmetic, stores ----
            for (int i0 = wt * 64 * UC; i0 < mp; i0 += 64 * UC * W) {
                uint8_t sb[UC];
                int d[UC];
                float cur[UC][DR], out[UC][DR];
#pragma unroll
                for (int u = 0; u < UC; ++u)
                    if (i0 + u * 64 < mp) {  // wave-uniform
                        const int i = i0 + u * 64 + lane;
                        sb[u] = sy[i];
                        d[u] = rdeg[i];
#pragma unroll
                        for (int k = 0; k < DR; ++k) cur[u][k] = M[k * mp + i];
                    }
#pragma unroll
                for (int u = 0; u < UC; ++u)
                    if (i0 + u * 64 < mp) {
                        int parity = sb[u] & 1;  // total_sgn = syndrome[i] + #{b2c <= 0}, parity only (bp.hpp:236-262)
                        float temp = FLT_MAX;
#pragma unroll
                        for (int k = 0; k < DR; ++k) {
                            if (cur[u][k] <= 0) parity ^= 1;
                            out[u][k] = temp;
                            const float ab = __builtin_fabsf(cur[u][k]);
                            if (ab < temp) temp = ab;
                        }
                        temp = FLT_MAX;
#pragma unroll
                        for (int k = DR - 1; k >= 0; --k) {
                            const int sgn = parity ^ (cur[u][k] <= 0 ? 1 : 0);
                            float mag = out[u][k];
                            if (temp < mag) mag = temp;
                            out[u][k] = mag * (sgn ? -alpha : alpha);
                            const float ab = __builtin_fabsf(cur[u][k]);
                            if (ab < temp) temp = ab;
                        }
                    }
#pragma unroll
                for (int u = 0; u < UC; ++u)
                    if (i0 + u * 64 < mp) {
                        const int i = i0 + u * 64 + lane;
#pragma unroll
                        for (int k = 0; k < DR; ++k) M[k < d[u] ? k * mp + i : DUMMY] = out[u][k];  // phantom entries keep their neutral value
                    }
            }
            team_sync();
            // ---- bit pass (bp.hpp:276-298, 311-318), in place through the position table, U bits per lane in flight ----
            for (int j0 = wt * 64 * U; j0 < np; j0 += 64 * U * W) {
                int pos[U][DC];
                float c[U][DC], pre[U][DC], pr[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j0 + u * 64 < np) {
                        const int j = j0 + u * 64 + lane;
                        pr[u] = a.prior_g[j];
#pragma unroll
                        for (int k = 0; k < DC; ++k) { pos[u][k] = apos[k * np + j]; c[u][k] = M[pos[u][k]]; }  // phantom: the +0.0f slot
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j0 + u * 64 < np) {
                        float temp = pr[u];
#pragma unroll
                        for (int k = 0; k < DC; ++k) { pre[u][k] = temp; temp += c[u][k]; }
                        if (want_llr) L[j0 + u * 64 + lane] = temp;
                        if (llr_direct && j0 + u * 64 + lane < n) a.llr[b * n + j0 + u * 64 + lane] = (double)temp;  // widened; the last pass's stay
                        const uint64_t word = __ballot(temp <= 0);  // padding bits: prior 1.0f, no entries -> 0
                        if (lane == 0) hardw[(j0 >> 6) + u] = word;
                        float sfx = 0.0f;
#pragma unroll
                        for (int k = DC - 1; k >= 0; --k) {
                            pre[u][k] = pre[u][k] + sfx;
                            sfx += c[u][k];
                        }
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j0 + u * 64 < np) {
#pragma unroll
                        for (int k = 0; k < DC; ++k) M[pos[u][k] == ZERO ? DUMMY : pos[u][k]] = pre[u][k];
                    }
            }
            team_sync();
            // ---- syndrome test (bp.hpp:292-294, 300-302): candidate parity of every check vs its syndrome BYTE ----
            bool unsat = false;
            for (int i0 = wt * 64; i0 < mp; i0 += 64 * W) {
                const int i = i0 + lane;
                unsigned par = 0;
#pragma unroll
                for (int k = 0; k < DR; ++k) {
                    const int cj = col[k * mp + i];  // phantom: bit np, always zero
                    par ^= (unsigned)(hardw[cj >> 6] >> (cj & 63)) & 1u;
                }
                unsat |= par != (unsigned)sy[i];
            }
            unsat_any = __ballot(unsat) != 0;
            if (TEAM) {  // (two flags: iteration it + 1 raises the other one, which nobody has read since iteration it - 1)
                if (unsat_any && lane == 0) team_unsat[it & 1] = 1;
                if (tid == 0) team_unsat[(it + 1) & 1] = 0;
                __syncthreads();
                unsat_any = team_unsat[it & 1] != 0;
            }
        } while (unsat_any && it < a.max_iter);

        // ---- outputs (bp.hpp:62,65,69,71) ----
        for (int j = tl; j < n; j += TS) {
            a.decoding[b * n + j] = (uint8_t)((hardw[j >> 6] >> (j & 63)) & 1ull);
            if (want_llr) a.llr[b * n + j] = (double)L[j];
        }
        if (tl == 0) {
            if (a.iters) a.iters[b] = it;
            if (a.conv) a.conv[b] = unsat_any ? 0 : 1;
        }
        team_sync();
    }
    if (threadIdx.x == 0) clock_probe_end(a.clk, clk_stamp);
}
