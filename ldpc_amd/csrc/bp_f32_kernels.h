// bp_f32_kernels.h -- float32 message mode (ldpc_hip_bp_set_message_dtype): min-sum, flooding schedule, one launch per pass
// Part of libldpc_hip.so (translation unit tu_f32.hip; host side: host_f32.h).
//
// The arithmetic contract ("float32 messages"; tests/f32_util.py restates it in NumPy and the GPU tests compare bit for bit):
//   * priors: the handle's FP64 log((1 - p) / p), rounded once to FP32 (round-to-nearest-even: v_cvt_f32_f64),
//   * messages: FP32, tile layout [tiles][nnz][64] -- an edge of a tile is one 256-byte segment,
//   * check pass: per edge the minimum of |bit_to_check| over the row's OTHER entries (FLT_MAX for a row of one entry), its sign from the
//     others' signs and the syndrome bit, times alpha in ONE FP32 multiply; alpha is formed in FP64 as in bp_spread_check_kernel and
//     rounded once to FP32,
//   * bit pass: the additions of the FP64 kernels (forward partial sums from the prior, backward partial sums from 0.0f, same operand
//     order), each ONE FP32 add; the posterior is the forward sum, the hard decision `posterior <= 0`,
//   * no FMA contraction, no reassociation, denormals kept: the unit is compiled with -ffp-contract=off (csrc/Makefile: CFLAGS, as every
//     unit) and repeats it below as a pragma; nothing here is built with fast-math.
// Structure: the per-pass family of bp_spread_kernels.h -- wavefronts spread over the nodes of all tiles, lane = syndrome, CSR / CSC
// tables from the handle, a device-side list of the running tiles that bp_f32_compact_kernel shortens -- with every kernel in the looping
// form (workgroup row y serves slots y, y + gridDim.y, ...), so that a launch stays small whatever the batch and rows without a tile leave
// at once.  One wavefront moves one edge (64 lanes x 4 B) per load instruction; two edges per instruction would need a cross-lane
// exchange for every value and was not built (DESIGN.md records the choice).
#pragma once

#include "bp_device_common.h"

#pragma clang fp contract(off)

struct F32Args {
    int32_t m, n, nnz, max_iter;
    double ms_scaling_factor;
    int64_t batch;                      // syndromes of this chunk (the last tile may be partial)
    const int32_t *row_ptr, *col_idx;   // CSR
    const int32_t *col_ptr, *csc_edge;  // CSC: CSR edge id of each column entry, rows ascending
    const float *llr0;                  // [n] priors, rounded from the handle's FP64 ones
    float *A;                           // bit_to_check  [tiles][nnz][64]
    float *C;                           // check_to_bit  [tiles][nnz][64]
    const uint64_t *par;                // [tiles][m]  bit l = syndrome byte & 1 of lane l
    const uint64_t *invalid;            // [tiles]     bit l = some syndrome byte > 1 (never converges)
    uint64_t *dec, *dcur;               // [tiles][n]  frozen / running hard decisions, bit l = lane l
    float *llr_t;                       // [tiles][n][64] posteriors, or nullptr
    int32_t *iters;                     // [batch] or nullptr
    uint8_t *conv;                      // [batch] or nullptr
    TileState *state;                   // [tiles]
    unsigned *counters;                 // [1] tiles in `list`, [2] tiles still running
    int32_t *list;                      // [tiles] the running tiles first (bp_f32_compact_kernel)
    int32_t nodes;                      // rows / columns per wavefront
    int32_t round;                      // 0-based and ABSOLUTE (a second pass starts at round0); the iteration is round + 1
    unsigned *host_flag;                // host-mapped word: receives `seq` when the last tile becomes final
    unsigned seq;
    // The two-pass decode (host_f32.h: decode_f32_repacked; the analogue of StreamPass::max_iter / keep_state and BpArgs::it_start, rows_dev, row_map).
    // pass_end: the iteration at which every tile of this pass ends.  == max_iter: a plain decode, or a second pass.  < max_iter: a first
    // pass whose state a second pass carries on -- max_iter stays the decode's own, so the bit pass of iteration pass_end still writes its
    // messages and the finish kernel reports the rows still decoding as conv = 0, iters = max_iter (the second pass overwrites both, and
    // their decisions and posteriors).  alpha and "the last iteration" keep using the absolute iteration and max_iter.
    int32_t pass_end;
    // round0: the rounds this pass's rows have behind them (0 unless a second pass): bp_f32_state_init_kernel writes the state a tile
    // reads in that round (done[round0 & 1]).  A second pass's A already holds the gathered bit_to_check state (bp_f32_gather_lanes_kernel).
    int32_t round0;
    // Rows known to the device only (a second pass).  rows_dev (if not null): [0] the rows of this pass, [1] their 64-row tiles (written
    // by repack_rows_kernel) -- they override `batch` and the host's tile count, whose grids follow an estimate (every kernel loops).
    // row_map (if not null): row r of the pass is row row_map[r] of the caller's `iters` / `conv`.
    const unsigned *rows_dev;
    const int32_t *row_map;
};

__device__ __forceinline__ int64_t f32_rows(const F32Args &a) {
    return a.rows_dev ? (int64_t)__hip_atomic_load(a.rows_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.batch;
}

// one tile's [rows][64] floats behind a buffer descriptor (as MsgBufT, for 4-byte elements): SGPR descriptor + SGPR edge offset +
// VGPR lane offset; an access outside the tile's rows reads 0 / is dropped.  AUX 2 = non-temporal.
template <int AUX>
struct MsgBuf32T {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ __forceinline__ float ld(int lane4, int edge) const {  // edge is wave-uniform
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, lane4, (int)((unsigned)edge << 8), AUX));
    }
    __device__ __forceinline__ void st(int lane4, int edge, float x) const {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), rsrc, lane4, (int)((unsigned)edge << 8), AUX);
    }
};
template <class BUF>
__device__ __forceinline__ BUF make_msgbuf32(float *base, unsigned rows) {
    BUF b;
    b.rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)(rows << 8), 0x00020000);
    return b;
}

// tile in `slot`, its iteration number and converged mask in this round; false: the tile is final
__device__ __forceinline__ bool f32_tile(const F32Args &a, int slot, int64_t &tile, const TileState *&st, int &it, uint64_t &done) {
    tile = a.list[slot];
    st = a.state + tile;
    it = a.round + 1;
    done = st->done[a.round & 1];
    return a.round <= st->end_round;
}

// n_tiles: the host's tile count (the grid covers it); a second pass takes rows and tiles from rows_dev -- never more than that.  A second
// pass without a row reports the decode finished itself: no finish kernel will (the host then stops queueing its rounds).
__global__ void __launch_bounds__(256) bp_f32_state_init_kernel(const F32Args a, int n_tiles) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows = f32_rows(a);
    if (a.rows_dev) {
        const int64_t tiles_dev = (rows + LDPC_WAVE - 1) / LDPC_WAVE;
        if (tiles_dev < n_tiles) n_tiles = (int)tiles_dev;
    }
    if (t == 0) {
        a.counters[1] = a.counters[2] = (unsigned)n_tiles;
        if (n_tiles == 0 && a.host_flag) __hip_atomic_store(a.host_flag, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (t >= n_tiles) return;
    TileState *st = a.state + t;
    const int64_t valid = rows - (int64_t)t * LDPC_WAVE;
    const int par = a.round0 & 1;
    st->done[par] = valid >= LDPC_WAVE ? 0ull : ~((1ull << valid) - 1ull);
    st->unsat[0] = st->unsat[1] = 0ull;
    st->it0 = 0;
    st->end_round = INT32_MAX;
    st->llr_each[par] = 0;
    for (int l = 0; l < 64; ++l) st->lane_iter[l] = 0;
    a.list[t] = t;
}

// the handle's FP64 priors, each rounded once to FP32
__global__ void __launch_bounds__(256) bp_f32_priors_kernel(const double *__restrict__ llr0, int n, float *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = (float)llr0[j];
}

// every edge starts with its column's prior (bp.hpp:147-157); grid (ceil(nnz / 64), tiles)
__global__ void __launch_bounds__(256) bp_f32_init_kernel(const F32Args a) {
    const int64_t tile = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const MsgBuf32T<0> At = make_msgbuf32<MsgBuf32T<0>>(a.A + (size_t)tile * (size_t)a.nnz * LDPC_WAVE, (unsigned)a.nnz);
    const int e0 = (blockIdx.x * 4 + wave) * 16;
    for (int e = e0; e < e0 + 16 && e < a.nnz; ++e) At.st(lane * 4, e, sload(a.llr0 + sload(a.col_idx + e)));
}

// The two-pass decode: the message state of the listed rows, lane by lane, out of the first pass's tiles into dense tiles -- the float32
// form of gather_lane_state_kernel (io_kernels.h).  Row list[r] (tile list[r] / 64, lane list[r] % 64) becomes lane r % 64 of tile r / 64;
// src, dst: [tiles][nnz][64] floats.  One wavefront per (destination tile, edge): 64 gathered 4-byte loads (the live lanes of a source
// tile share sectors), one coalesced 256-byte store; lanes beyond the count are written 0.  The count is the device's (rows_dev[0]), the
// grid an estimate: workgroup row y serves tiles y, y + gridDim.y, ...  grid (ceil(nnz / (4 * edges_per_wave)), estimate).
__global__ void __launch_bounds__(256) bp_f32_gather_lanes_kernel(const float *__restrict__ src, const int32_t *__restrict__ list, const unsigned *__restrict__ rows_dev,
                                                                  int nnz, int edges_per_wave, float *__restrict__ dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t count = (int64_t)__hip_atomic_load(rows_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int64_t tile = blockIdx.y; tile * LDPC_WAVE < count; tile += gridDim.y) {
        const int64_t r = tile * LDPC_WAVE + lane;
        const bool live = r < count;
        const int64_t b = live ? (int64_t)list[r] : 0;
        const float *from = src + ((b >> 6) * (int64_t)nnz) * LDPC_WAVE + (b & 63);
        float *to = dst + (tile * (int64_t)nnz) * LDPC_WAVE + lane;
        const int e0 = (blockIdx.x * 4 + wave) * edges_per_wave;
        for (int e = e0; e < e0 + edges_per_wave && e < nnz; ++e) to[(int64_t)e * LDPC_WAVE] = live ? from[(int64_t)e * LDPC_WAVE] : 0.0f;
    }
}

// the list without the tiles that are final (in place, one wavefront; counters[1] = how many are left)
__global__ void __launch_bounds__(64) bp_f32_compact_kernel(const F32Args a) {
    const int lane = threadIdx.x;
    const int n_tiles = (int)a.counters[1];
    int kept = 0;
    for (int s0 = 0; s0 < n_tiles; s0 += 64) {  // (a chunk is read whole before any of it is overwritten: kept <= s0)
        const int slot = s0 + lane;
        int32_t tile = 0;
        bool live = false;
        if (slot < n_tiles) {
            tile = a.list[slot];
            live = a.round <= a.state[tile].end_round;
        }
        const uint64_t mask = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        if (live) a.list[kept + lane_rank(mask)] = tile;
        kept += __builtin_popcountll(mask);
    }
    if (lane == 0) a.counters[1] = (unsigned)kept;
}

// check pass (bp.hpp:220-273 in FP32): rows of up to DR entries in registers, heavier ones in two sweeps through memory
template <int DR, int NT>
__global__ void __launch_bounds__(256) bp_f32_check_kernel(const F32Args a) {
    typedef MsgBuf32T<NT ? 2 : 0> Buf;
    const int lane = threadIdx.x & 63, l4 = lane * 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int count = (int)a.counters[1];
    const int nnz = a.nnz;
    for (int slot = blockIdx.y; slot < count; slot += gridDim.y) {
        int64_t tile;
        const TileState *st;
        int it;
        uint64_t done;
        if (!f32_tile(a, slot, tile, st, it, done)) continue;  // (uniform over the workgroup)
        const Buf At = make_msgbuf32<Buf>(a.A + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
        const Buf Ct = make_msgbuf32<Buf>(a.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
        const float alpha = (float)((a.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.ms_scaling_factor);
        const int i0 = (blockIdx.x * 4 + wave) * a.nodes;
        for (int i = i0; i < i0 + a.nodes && i < a.m; ++i) {
            const int rs = sload(a.row_ptr + i), d = sload(a.row_ptr + i + 1) - rs;
            int parity = (int)((sload(a.par + tile * a.m + i) >> lane) & 1ull);
            if (d <= DR) {
                float cur[DR], pre[DR];
#pragma unroll
                for (int k = 0; k < DR; ++k)
                    if (k < d) cur[k] = At.ld(l4, rs + k);
                float temp = FLT_MAX;
#pragma unroll
                for (int k = 0; k < DR; ++k)
                    if (k < d) {
                        if (cur[k] <= 0) parity ^= 1;
                        pre[k] = temp;
                        const float ab = fabsf(cur[k]);
                        if (ab < temp) temp = ab;
                    }
                temp = FLT_MAX;
#pragma unroll
                for (int k = DR - 1; k >= 0; --k)
                    if (k < d) {
                        const int sgn = parity ^ (cur[k] <= 0 ? 1 : 0);
                        float mag = pre[k];
                        if (temp < mag) mag = temp;
                        Ct.st(l4, rs + k, mag * (sgn ? -alpha : alpha));
                        const float ab = fabsf(cur[k]);
                        if (ab < temp) temp = ab;
                    }
            } else {
                float temp = FLT_MAX;
                for (int k = 0; k < d; ++k) {
                    const float bk = At.ld(l4, rs + k);
                    if (bk <= 0) parity ^= 1;
                    Ct.st(l4, rs + k, temp);
                    const float ab = fabsf(bk);
                    if (ab < temp) temp = ab;
                }
                temp = FLT_MAX;
                for (int k = d - 1; k >= 0; --k) {
                    const float bk = At.ld(l4, rs + k);
                    const int sgn = parity ^ (bk <= 0 ? 1 : 0);
                    float mag = Ct.ld(l4, rs + k);
                    if (temp < mag) mag = temp;
                    Ct.st(l4, rs + k, mag * (sgn ? -alpha : alpha));
                    const float ab = fabsf(bk);
                    if (ab < temp) temp = ab;
                }
            }
        }
    }
}

// bit pass (bp.hpp:276-287, 311-318 in FP32): columns of up to DC entries in registers, heavier ones in the reference's two sweeps
template <int DC, int NT>
__global__ void __launch_bounds__(256) bp_f32_bit_kernel(const F32Args a) {
    typedef MsgBuf32T<NT ? 2 : 0> Buf;
    const int lane = threadIdx.x & 63, l4 = lane * 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int count = (int)a.counters[1];
    const int nnz = a.nnz, n = a.n;
    const bool want_llr = a.llr_t != nullptr;
    for (int slot = blockIdx.y; slot < count; slot += gridDim.y) {
        int64_t tile;
        const TileState *st;
        int it;
        uint64_t done;
        if (!f32_tile(a, slot, tile, st, it, done)) continue;
        const Buf At = make_msgbuf32<Buf>(a.A + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
        const Buf Ct = make_msgbuf32<Buf>(a.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
        const Buf Lt = make_msgbuf32<Buf>(want_llr ? a.llr_t + (size_t)tile * (size_t)n * LDPC_WAVE : a.A, want_llr ? (unsigned)n : 0u);
        const bool last = it == a.max_iter;  // (nobody reads the messages of the last bit pass)
        const bool lane_live = !((done >> lane) & 1ull);
        const bool each = st->llr_each[a.round & 1] != 0;
        const int j0 = (blockIdx.x * 4 + wave) * a.nodes;
        for (int j = j0; j < j0 + a.nodes && j < n; ++j) {
            const int cs = sload(a.col_ptr + j), d = sload(a.col_ptr + j + 1) - cs;
            const float prior = sload(a.llr0 + j);
            float llr;
            if (d <= DC) {
                int e[DC];
                float c[DC], pre[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k)
                    if (k < d) { e[k] = sload(a.csc_edge + cs + k); c[k] = Ct.ld(l4, e[k]); }
                float temp = prior;
#pragma unroll
                for (int k = 0; k < DC; ++k)
                    if (k < d) { pre[k] = temp; temp += c[k]; }
                llr = temp;
                if (!last) {
                    float s = 0.0f;
#pragma unroll
                    for (int k = DC - 1; k >= 0; --k)
                        if (k < d) { At.st(l4, e[k], pre[k] + s); s += c[k]; }
                }
            } else {
                float temp = prior;
                for (int k = 0; k < d; ++k) {
                    const int ee = sload(a.csc_edge + cs + k);
                    At.st(l4, ee, temp);
                    temp += Ct.ld(l4, ee);
                }
                llr = temp;
                float sfx = 0.0f;
                for (int k = d - 1; k >= 0; --k) {
                    const int ee = sload(a.csc_edge + cs + k);
                    At.st(l4, ee, At.ld(l4, ee) + sfx);
                    sfx += Ct.ld(l4, ee);
                }
            }
            const uint64_t hard = __ballot(llr <= 0);
            if (lane == 0) a.dcur[tile * n + j] = hard;
            if ((last || each) && want_llr && lane_live) Lt.st(l4, j, llr);
        }
    }
}

// candidate syndrome against the syndrome (bp.hpp:292-302), one thread per (tile, row); OR-accumulated into TileState::unsat
__global__ void __launch_bounds__(256) bp_f32_synd_kernel(const F32Args a) {
    const int count = (int)a.counters[1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    for (int slot = blockIdx.y; slot < count; slot += gridDim.y) {
        int64_t tile;
        const TileState *st;
        int it;
        uint64_t done;
        if (!f32_tile(a, slot, tile, st, it, done)) continue;
        uint64_t unsat = 0;
        if (i < a.m) {
            const uint64_t *dcur = a.dcur + tile * a.n;
            uint64_t cand = 0;
            for (int e = a.row_ptr[i]; e < a.row_ptr[i + 1]; ++e) cand ^= dcur[a.col_idx[e]];
            unsat = cand ^ a.par[tile * a.m + i];
        }
        unsat = wave_or(unsat);
        if ((threadIdx.x & 63) == 0 && unsat) atomicOr(&a.state[tile].unsat[a.round & 1], (unsigned long long)unsat);
    }
}

// convergence bookkeeping of a round (bp.hpp:296-311, 320-322), as bp_spread_finish_kernel: lanes whose candidate syndrome matched are
// frozen (decisions + posterior of THIS iteration), a tile whose lanes are all frozen or that reached max_iter gets its outputs.
// 64 bits per workgroup; workgroup 0 of a tile also advances its state.
__global__ void __launch_bounds__(256) bp_f32_finish_kernel(const F32Args a) {
    const int count = (int)a.counters[1];
    const int par = a.round & 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n, nnz = a.nnz, l4 = lane * 4;
    const bool want_llr = a.llr_t != nullptr;
    for (int slot = blockIdx.y; slot < count; slot += gridDim.y) {
        int64_t tile;
        const TileState *cst;
        int it;
        uint64_t done;
        if (!f32_tile(a, slot, tile, cst, it, done)) continue;
        TileState *st = a.state + tile;
        const bool last = it == a.max_iter;
        const uint64_t unsat = cst->unsat[par] | a.invalid[tile];
        const uint64_t newly = ~unsat & ~done;
        const uint64_t ndone = done | newly;
        const bool over = ndone == ~0ull || it == a.pass_end;  // (pass_end < max_iter: a first pass -- the rows still decoding leave as unconverged, for the second)
        const bool mine = (newly >> lane) & 1ull;
        const bool each = cst->llr_each[par] != 0;
        if (newly || (over && ndone != ~0ull)) {
            uint64_t *dec = a.dec + tile * n;
            const uint64_t *dcur = a.dcur + tile * n;
            const MsgBuf32T<0> Ct = make_msgbuf32<MsgBuf32T<0>>(a.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
            const MsgBuf32T<0> Lt = make_msgbuf32<MsgBuf32T<0>>(want_llr ? a.llr_t + (size_t)tile * (size_t)n * LDPC_WAVE : a.A, want_llr ? (unsigned)n : 0u);
            const int j0 = blockIdx.x * 64 + wave * 16;
            for (int j = j0; j < j0 + 16 && j < n; ++j) {
                if (lane == 0) {
                    const uint64_t cur = dcur[j];
                    uint64_t d = (dec[j] & ~newly) | (cur & newly);
                    if (over) d = (d & ndone) | (cur & ~ndone);  // never converged: the last iteration's decisions
                    dec[j] = d;
                }
                if (newly && !last && want_llr && !each) {  // (at the last iteration, or under llr_each, the bit pass has stored the posterior already)
                    float temp = a.llr0[j];
                    for (int p = a.col_ptr[j]; p < a.col_ptr[j + 1]; ++p) temp += Ct.ld(l4, a.csc_edge[p]);
                    if (mine) Lt.st(l4, j, temp);
                }
            }
        }
        if (blockIdx.x != 0) continue;
        if (wave == 0) {
            const int earlier = st->lane_iter[lane];
            if (mine) st->lane_iter[lane] = it;
            const int64_t r = tile * LDPC_WAVE + lane;
            if (over && r < f32_rows(a)) {
                const int64_t b = a.row_map ? (int64_t)a.row_map[r] : r;
                const bool cv = ((ndone >> lane) & 1ull) != 0;
                if (a.iters) a.iters[b] = cv ? (mine ? it : earlier) : a.max_iter;  // bp.hpp:304
                if (a.conv) a.conv[b] = cv ? 1 : 0;
            }
        }
        if (threadIdx.x == 0) {
            st->done[par ^ 1] = ndone;
            st->unsat[par ^ 1] = 0ull;
            st->llr_each[par ^ 1] = (each || newly) ? 1 : 0;  // after the first event: every bit pass stores the live lanes' posteriors
            if (over) {
                st->end_round = a.round;
                if (atomicSub(&a.counters[2], 1u) == 1u && a.host_flag)  // that was the last live tile
                    __hip_atomic_store(a.host_flag, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// llr_t [tiles][n][64] f32 -> llr [batch][n] f64 (each value widened exactly), 64 x 64 tiles through LDS; grid (ceil(n / 64), tiles)
// row_map / count_dev: rows known to the device only, as transpose_llr_kernel takes them (io_kernels.h) -- grid.y is then an estimate, so the kernel loops over the tiles
__global__ void __launch_bounds__(256) bp_f32_transpose_llr_kernel(const float *__restrict__ llr_t, int64_t batch_arg, int n, double *out,
                                                                   const int32_t *__restrict__ row_map, const unsigned *count_dev) {
    __shared__ float tilebuf[LDPC_WAVE][LDPC_WAVE + 1];
    const int j0 = blockIdx.x * LDPC_WAVE;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    const int64_t batch = count_dev ? (int64_t)__hip_atomic_load(count_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : batch_arg;
    for (int64_t tile = blockIdx.y; tile * LDPC_WAVE < batch; tile += gridDim.y) {
        for (int r = 0; r < 16; ++r) {
            const int jj = r * 4 + hi;
            if (j0 + jj < n) tilebuf[jj][lo] = llr_t[((size_t)tile * n + j0 + jj) * LDPC_WAVE + lo];
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {
            const int l = r * 4 + hi;
            const int64_t b = tile * LDPC_WAVE + l;
            if (b < batch && j0 + lo < n) out[(size_t)(row_map ? (int64_t)row_map[b] : b) * n + j0 + lo] = (double)tilebuf[lo][l];
        }
        __syncthreads();  // (the buffer is refilled for the next tile)
    }
}
