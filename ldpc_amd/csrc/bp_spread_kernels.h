// bp_spread_kernels.h -- per-pass kernels: check pass, bit pass, syndrome test and bookkeeping spread over the whole chip
// Part of libldpc_hip.so (one translation unit: bp_hip.hip includes every kernel header).
#pragma once

#include "bp_device_common.h"
#include "relay_common.h"

// ---- per-pass kernels for handed-off tiles ---------------------------------------------------------------
// Same arithmetic, same arrays, but one launch per pass and one wavefront per NODE, so the rows / columns of a
// single tile are spread over all 256 compute units.  Used for the tiles the persistent kernel parks when the
// chip would otherwise idle; each launch handles every parked tile that is still running.
struct SpreadArgs {
    BpArgs bp;
    int32_t n_tiles;  // entries of bp.handoff_list; < 0: only the device knows (bp.counters[1], left by the persistent kernel)
    int32_t nodes;    // rows / columns per wavefront (1 for a handful of tiles: latency; 4, or 16 for >= 512 tiles from the start: amortises the table load)
    int32_t round;    // 0-based per-pass round; a tile's iteration number is it0 + round + 1
    unsigned *host_flag;  // host-mapped word: receives `seq` when the last parked tile becomes final (the host stops queueing rounds)
    unsigned seq;
    int32_t slot0;    // the first slot of the list this launch serves (workgroup row y: slot0 + y; the LOOP forms: and every gridDim.y-th after it)
    // Row priors (the <..., RP> forms; io_kernels.h: row_priors_kernel): [tiles][n][64] log((1 - p) / p) of every lane's OWN channel
    // probabilities, in the layout of the messages -- the reference's `update_channel_probs(p[shot]); decode(s[shot])` loop
    // (_bp_decoder.pyx:222) as one batch.  Read where the other forms read bp.llr0[j]; nullptr otherwise.
    const double *llr0_t;
    // Memory min-sum (the bp_spread_mem_* kernels): llr0_t is then M [tiles][n][64], every lane's posterior of the previous
    // iteration (the prior log-ratio to begin with: bp_spread_mem_init_kernel), read AND rewritten by every bit pass for all 64 lanes; mem_ag [2][n]
    // = a[] = (1 - gamma) * llr0, then gamma[] (mem_host.h), read per column through the scalar path as llr0 is.  nullptr otherwise.
    const double *mem_ag;
    // Relay-BP, a leg after the first (bp_spread_relay_init_kernel): [bp.batch][n] row-major, the previous leg's posteriors of
    // this chunk's rows -- what M starts from instead of the prior log-ratios.  nullptr otherwise.
    const double *relay_seed;
};

// the prior of column j's bit pass under memory: llr0[j] where gamma[j] == 0 (a select: a[j] IS llr0[j] there, infinities included), else
// a[j] + gamma[j] * M -- the product rounded, then the sum (no FMA: -ffp-contract=off)
__device__ __forceinline__ double mem_prior(const double *mem_ag, int n, int j, double m_prev) {
    const double aj = sload(mem_ag + j), g = sload(mem_ag + n + j);
    return g == 0.0 ? aj : aj + g * m_prev;
}

// Late rounds.  After a few rounds all but a handful of the tiles are final (what is left is what never converges), yet a launch of a row of
// workgroups per parked tile -- 256 rows that leave at once -- costs ~50 us, four times a round, for the 40 rounds one hopeless syndrome keeps
// its tile going.  Where the host expects that (host_stream.h) the list is compacted on the device every 8 rounds (bp_spread_compact_kernel:
// the running tiles to the front) and a round is then TWO launches per kernel: 32 rows for slots 0 .. 31, exactly as before, and 8 rows of
// the LOOP form for whatever lies beyond (slot0 = 32: every 8th slot each; nothing, normally -- they leave at once).  The row-per-slot form
// stays as it was: with a loop over slots in it the check kernel needed 109 VGPRs instead of 73 and the headline lost 3 %.
__device__ __forceinline__ int spread_count(const SpreadArgs &a) { return a.n_tiles >= 0 ? a.n_tiles : (int)a.bp.counters[1]; }

// the list without the tiles that are final (in place, one wavefront; counters[1] = how many are left)
__global__ void __launch_bounds__(64) bp_spread_compact_kernel(const SpreadArgs a) {
    const int lane = threadIdx.x;
    const int n_tiles = spread_count(a);
    int kept = 0;
    for (int s0 = 0; s0 < n_tiles; s0 += 64) {  // (a chunk is read whole before any of it is overwritten: kept <= s0)
        const int slot = s0 + lane;
        int32_t tile = 0;
        bool live = false;
        if (slot < n_tiles) {
            tile = a.bp.handoff_list[slot];
            live = a.round <= a.bp.state[tile].end_round;
        }
        const uint64_t mask = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        if (live) a.bp.handoff_list[kept + lane_rank(mask)] = tile;
        kept += __builtin_popcountll(mask);
    }
    if (lane == 0) a.bp.counters[1] = (unsigned)kept;
}

// tile in `slot`, its iteration number and converged mask in this round; false: no such slot, or the tile is final
__device__ __forceinline__ bool spread_tile(const SpreadArgs &a, int slot, int64_t &tile, const TileState *&st, int &it, uint64_t &done) {
    // The host sizes the grid for the most tiles that can have been parked and queues every round without waiting for
    // the device (the *_async entry points never synchronise): rows beyond the parked count and tiles that are final leave here.
    if (slot >= spread_count(a)) return false;
    tile = a.bp.handoff_list[slot];
    st = a.bp.state + tile;
    it = st->it0 + a.round + 1;
    done = st->done[a.round & 1];
    return a.round <= st->end_round;
}


template <int METHOD, int MATH, int DR, int NT, bool LOOP = false>
__global__ void __launch_bounds__(256) bp_spread_check_kernel(const SpreadArgs a) {
    typedef MsgBufT<NT ? 2 : 0> Buf;  // cache policy of the message traffic: non-temporal once the tiles outgrow the caches
    __shared__ __attribute__((aligned(16))) double log_tab[256];
    __shared__ double near_bufs[4][LDPC_NEAR_SLOTS];
    int64_t tile;
    const TileState *st;
    int it;
    uint64_t done;
    int slot = a.slot0 + (int)blockIdx.y;
    if (LOOP) { if (slot >= spread_count(a)) return; }
    else if (!spread_tile(a, slot, tile, st, it, done)) return;  // (uniform over the workgroup)
    if (METHOD == LDPC_HIP_PRODUCT_SUM && MATH == 0)
        for (int q = threadIdx.x; q < 256; q += blockDim.x) log_tab[q] = ldpc_math::k_log_tab[q];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nnz = a.bp.nnz, l8 = lane * 8;
    do {
    if (LOOP && !spread_tile(a, slot, tile, st, it, done)) continue;
    const Buf At = make_msgbuf<Buf>(a.bp.A + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
    const Buf Ct = make_msgbuf<Buf>(a.bp.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
    const double alpha = (a.bp.ms_scaling_factor == 0.0) ? 1.0 - ldexp(1.0, -it) : a.bp.ms_scaling_factor;
    const int i0 = (blockIdx.x * 4 + wave) * a.nodes;
    for (int i = i0; i < i0 + a.nodes && i < a.bp.m; ++i) {
        const int rs = sload(a.bp.row_ptr + i), d = sload(a.bp.row_ptr + i + 1) - rs;
        const bool neg = (sload(a.bp.nzm + tile * a.bp.m + i) >> lane) & 1ull;
        const int parity = (int)((sload(a.bp.par + tile * a.bp.m + i) >> lane) & 1ull);
        if (d <= DR) {
            double cur[DR];
#pragma unroll
            for (int k = 0; k < DR; ++k)
                if (k < d) cur[k] = At.ld(l8, rs + k);
            check_row_live<METHOD, MATH, DR>(cur, d, rs, neg, parity, alpha, Ct, l8, log_tab, ~done, near_bufs[wave]);
        } else {
            check_row_streamed<METHOD, MATH>(d, rs, neg, parity, alpha, At, Ct, l8, log_tab);
        }
    }
    } while (LOOP && (slot += (int)gridDim.y) < spread_count(a));
}

// (the body of bp_spread_bit_kernel and of its memory form bp_spread_mem_bit_kernel: MEM -- memory min-sum, see SpreadArgs::mem_ag)
template <int METHOD, int MATH, int DC, int NT, bool LOOP, bool RP, bool MEM>
__device__ __forceinline__ void spread_bit_pass(const SpreadArgs &a) {
    static_assert(!(RP && MEM), "row priors and memory exclude each other (both live in llr0_t)");
    typedef MsgBufT<NT ? 2 : 0> Buf;
    int64_t tile;
    const TileState *st;
    int it;
    uint64_t done;
    int slot = a.slot0 + (int)blockIdx.y;
    if (LOOP) { if (slot >= spread_count(a)) return; }
    else if (!spread_tile(a, slot, tile, st, it, done)) return;
    do {
    if (LOOP && !spread_tile(a, slot, tile, st, it, done)) continue;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nnz = a.bp.nnz, n = a.bp.n, l8 = lane * 8;
    const Buf At = make_msgbuf<Buf>(a.bp.A + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
    const Buf Ct = make_msgbuf<Buf>(a.bp.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
    const bool want_llr = a.bp.llr_t != nullptr;
    const Buf Lt = make_msgbuf<Buf>(want_llr ? a.bp.llr_t + (size_t)tile * (size_t)n * LDPC_WAVE : a.bp.A, want_llr ? (unsigned)n : 0u);
    const Buf Pt = make_msgbuf<Buf>(RP || MEM ? const_cast<double *>(a.llr0_t) + (size_t)tile * (size_t)n * LDPC_WAVE : a.bp.A, RP || MEM ? (unsigned)n : 0u);
    const bool last = it == a.bp.max_iter;
    const bool lane_live = !((done >> lane) & 1ull);
    const bool each = st->llr_each[a.round & 1] != 0;  // (as the persistent kernel's llr_each)
    const int j0 = (blockIdx.x * 4 + wave) * a.nodes;
    for (int j = j0; j < j0 + a.nodes && j < n; ++j) {
        const int cs = sload(a.bp.col_ptr + j), d = sload(a.bp.col_ptr + j + 1) - cs;
        const double prior = MEM ? mem_prior(a.mem_ag, n, j, Pt.ld(l8, j))  // (MEM: from this lane's previous posterior)
                           : RP ? Pt.ld(l8, j) : sload(a.bp.llr0 + j);      // (RP: this lane's own prior)
        double llr;
        if (d <= DC) {
            int e[DC];
            double c[DC];
#pragma unroll
            for (int k = 0; k < DC; ++k)
                if (k < d) { e[k] = sload(a.bp.csc_edge + cs + k); c[k] = Ct.ld(l8, e[k]); }
            llr = bit_column<METHOD, MATH, DC>(c, e, d, prior, At, l8, !last || a.bp.keep_state != 0);
        } else {  // the reference's two sweeps (bp.hpp:278-281, 313-316) through memory
            double temp = prior;
            for (int k = 0; k < d; ++k) {
                const int ee = sload(a.bp.csc_edge + cs + k);
                At.st(l8, ee, temp);
                temp += Ct.ld(l8, ee);
            }
            llr = temp;
            double sfx = 0.0;
            for (int k = d - 1; k >= 0; --k) {
                const int ee = sload(a.bp.csc_edge + cs + k);
                At.st(l8, ee, edge_form<METHOD, MATH>(At.ld(l8, ee) + sfx));
                sfx += Ct.ld(l8, ee);
            }
        }
        if (MEM) Pt.st(l8, j, llr);  // M: every lane, whatever llr_each says (a column belongs to one wavefront: nobody else reads or writes it this pass)
        const uint64_t hard = __ballot(llr <= 0);
        if (lane == 0) a.bp.dcur[tile * n + j] = hard;
        if ((last || each) && want_llr && lane_live) Lt.st(l8, j, llr);
    }
    } while (LOOP && (slot += (int)gridDim.y) < spread_count(a));
}

template <int METHOD, int MATH, int DC, int NT, bool LOOP = false, bool RP = false>
__global__ void __launch_bounds__(256) bp_spread_bit_kernel(const SpreadArgs a) { spread_bit_pass<METHOD, MATH, DC, NT, LOOP, RP, false>(a); }

// Memory min-sum (minimum-sum only, never a compacted pass: no LOOP form): both column paths -- d <= DC in registers, d > DC in two sweeps
// through memory -- start from the prior formed from M and leave the posterior in M.
template <int DC, int NT>
__global__ void __launch_bounds__(256) bp_spread_mem_bit_kernel(const SpreadArgs a) { spread_bit_pass<LDPC_HIP_MINIMUM_SUM, 0, DC, NT, false, false, true>(a); }

// candidate syndrome vs syndrome (bp.hpp:292-294, 300-302) for the parked tiles, one thread per (tile, row); the
// per-tile verdict is OR-accumulated into TileState::unsat for bp_spread_finish_kernel
template <bool LOOP = false>
__global__ void __launch_bounds__(256) bp_spread_synd_kernel(const SpreadArgs a) {
    int64_t tile;
    const TileState *st;
    int it;
    uint64_t done;
    int slot = a.slot0 + (int)blockIdx.y;
    if (LOOP) { if (slot >= spread_count(a)) return; }
    else if (!spread_tile(a, slot, tile, st, it, done)) return;
    do {
    if (LOOP && !spread_tile(a, slot, tile, st, it, done)) continue;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t unsat = 0;
    if (i < a.bp.m) {
        const uint64_t *dcur = a.bp.dcur + tile * a.bp.n;
        uint64_t cand = 0;
        for (int e = a.bp.row_ptr[i]; e < a.bp.row_ptr[i + 1]; ++e) cand ^= dcur[a.bp.col_idx[e]];
        unsat = cand ^ a.bp.par[tile * a.bp.m + i];
    }
    unsat = wave_or(unsat);
    if ((threadIdx.x & 63) == 0 && unsat) atomicOr(&a.bp.state[tile].unsat[a.round & 1], (unsigned long long)unsat);
    } while (LOOP && (slot += (int)gridDim.y) < spread_count(a));
}

// batches of only a few tiles skip the persistent kernel altogether: state + message initialisation for the per-pass path
__global__ void __launch_bounds__(256) bp_spread_state_init_kernel(const SpreadArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_tiles) return;
    TileState *st = a.bp.state + t;
    const int64_t valid = a.bp.batch - (int64_t)t * LDPC_WAVE;
    st->done[0] = valid >= LDPC_WAVE ? 0ull : ~((1ull << valid) - 1ull);
    st->unsat[0] = st->unsat[1] = 0ull;
    st->it0 = a.bp.it_start;
    st->end_round = INT32_MAX;
    // lanes compacted out of a first pass (it_start > 0) are the ones about to converge: store their posteriors in every bit pass from
    // the start instead of paying a sweep over C per convergence event (1.3 ms per round on the headline code at p = 0.05)
    st->llr_each[0] = a.bp.it_start > 0 ? 1 : 0;
    for (int l = 0; l < 64; ++l) st->lane_iter[l] = 0;
    a.bp.handoff_list[t] = t;
    if (t == 0) a.bp.counters[1] = a.bp.counters[2] = (unsigned)a.n_tiles;  // parked, live
}

// (MEM: the initial messages are the plain ones; M starts as the prior log-ratio in every lane)
// (SEED, with MEM -- a leg of Relay-BP after the first: M starts as the lane's row of relay_seed, the previous leg's posteriors, and the initial
// message of every entry of column j is the prior the first bit pass will form from it, mem_prior(j, M) -- a[j] = L0[j] itself where gamma[j] == 0.
// Lanes beyond the batch in a ragged last tile take the prior log-ratios: nothing of them is ever read back.)
template <int METHOD, int MATH, bool RP, bool MEM, bool SEED = false>
__device__ __forceinline__ void spread_init(const SpreadArgs &a) {  // bp.hpp:147-157
    static_assert(!SEED || MEM, "a seeded start is a memory decode");
    const int64_t tile = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nnz = a.bp.nnz, l8 = lane * 8;
    const MsgBuf At = make_msgbuf(a.bp.A + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
    const MsgBuf Pt = make_msgbuf(RP ? const_cast<double *>(a.llr0_t) + (size_t)tile * (size_t)a.bp.n * LDPC_WAVE : a.bp.A, RP ? (unsigned)a.bp.n : 0u);
    const int e0 = (blockIdx.x * 4 + wave) * 16;
    const int64_t row = tile * LDPC_WAVE + lane;  // (SEED) this lane's row of the chunk
    const bool seeded = SEED && row < a.bp.batch;
    const double *seed = SEED ? a.relay_seed + (seeded ? row : 0) * (int64_t)a.bp.n : nullptr;
    for (int e = e0; e < e0 + 16 && e < nnz; ++e) {
        const int j = sload(a.bp.col_idx + e);
        if (SEED) At.st(l8, e, mem_prior(a.mem_ag, a.bp.n, j, seeded ? seed[j] : sload(a.bp.llr0 + j)));
        else At.st(l8, e, edge_form<METHOD, MATH>(RP ? Pt.ld(l8, j) : sload(a.bp.llr0 + j)));
    }
    if (MEM) {  // the same grid covers the columns: 64 per workgroup, nnz >= n where every column has an entry -- and a loop where not
        const MsgBuf Mt = make_msgbuf(const_cast<double *>(a.llr0_t) + (size_t)tile * (size_t)a.bp.n * LDPC_WAVE, (unsigned)a.bp.n);
        for (int j0 = (blockIdx.x * 4 + wave) * 16; j0 < a.bp.n; j0 += (int)gridDim.x * 64)
            for (int j = j0; j < j0 + 16 && j < a.bp.n; ++j) Mt.st(l8, j, seeded ? seed[j] : sload(a.bp.llr0 + j));
    }
}

template <int METHOD, int MATH, bool RP = false>
__global__ void __launch_bounds__(256) bp_spread_init_kernel(const SpreadArgs a) { spread_init<METHOD, MATH, RP, false>(a); }

__global__ void __launch_bounds__(256) bp_spread_mem_init_kernel(const SpreadArgs a) { spread_init<LDPC_HIP_MINIMUM_SUM, 0, false, true>(a); }

__global__ void __launch_bounds__(256) bp_spread_relay_init_kernel(const SpreadArgs a) { spread_init<LDPC_HIP_MINIMUM_SUM, 0, false, true, true>(a); }

// [n] initial edge values for BpArgs::edge0
template <int METHOD, int MATH>
__global__ void __launch_bounds__(256) bp_edge0_kernel(const double *llr0, int n, double *out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = edge_form<METHOD, MATH>(llr0[j]);
}

// convergence bookkeeping of a round (bp.hpp:296-311, 320-322): lanes whose candidate syndrome matched are frozen
// (decisions + posterior of THIS iteration), a tile whose lanes are all frozen or that reached max_iter gets its
// outputs.  64 bits per workgroup; workgroup 0 of a tile also advances its state.  Almost always there is nothing
// to freeze and every workgroup but the first leaves at once.
// (MEM: the posterior of THIS iteration is what the bit pass has just left in M -- the prior it used is gone, and there is nothing to add up)
template <bool LOOP, bool RP, bool MEM>
__device__ __forceinline__ void spread_finish(const SpreadArgs &a) {
    int64_t tile;
    const TileState *cst;
    int it;
    uint64_t done;
    int slot = a.slot0 + (int)blockIdx.y;
    if (LOOP) { if (slot >= spread_count(a)) return; }
    else if (!spread_tile(a, slot, tile, cst, it, done)) return;
    do {
    if (LOOP && !spread_tile(a, slot, tile, cst, it, done)) continue;
    TileState *st = a.bp.state + tile;
    const int par = a.round & 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.bp.n, nnz = a.bp.nnz, l8 = lane * 8;
    const bool last = it == a.bp.max_iter;
    const uint64_t unsat = cst->unsat[par] | a.bp.invalid[tile];
    const uint64_t newly = ~unsat & ~done;
    const uint64_t ndone = done | newly;
    const bool over = ndone == ~0ull || last;
    const bool mine = (newly >> lane) & 1ull;
    const bool each = cst->llr_each[par] != 0;
    if (newly || (over && ndone != ~0ull)) {
        uint64_t *dec = a.bp.dec + tile * n;
        const uint64_t *dcur = a.bp.dcur + tile * n;
        const MsgBuf Ct = make_msgbuf(a.bp.C + (size_t)tile * (size_t)nnz * LDPC_WAVE, (unsigned)nnz);
        const bool want_llr = a.bp.llr_t != nullptr;
        const MsgBuf Lt = make_msgbuf(want_llr ? a.bp.llr_t + (size_t)tile * (size_t)n * LDPC_WAVE : a.bp.A, want_llr ? (unsigned)n : 0u);
        const MsgBuf Pt = make_msgbuf(RP || MEM ? const_cast<double *>(a.llr0_t) + (size_t)tile * (size_t)n * LDPC_WAVE : a.bp.A, RP || MEM ? (unsigned)n : 0u);
        const int j0 = blockIdx.x * 64 + wave * 16;
        for (int j = j0; j < j0 + 16 && j < n; ++j) {
            if (lane == 0) {
                const uint64_t cur = dcur[j];
                uint64_t d = (dec[j] & ~newly) | (cur & newly);
                if (over) d = (d & ndone) | (cur & ~ndone);  // never converged: the last iteration's decisions
                dec[j] = d;
            }
            if (newly && !last && want_llr && !each) {  // (at the last iteration, or under llr_each, the bit pass has stored the posterior already)
                double temp = RP || MEM ? Pt.ld(l8, j) : a.bp.llr0[j];
                if (!MEM)
                    for (int p = a.bp.col_ptr[j]; p < a.bp.col_ptr[j + 1]; ++p) temp += Ct.ld(l8, a.bp.csc_edge[p]);
                if (mine) Lt.st(l8, j, temp);
            }
        }
    }
    if (blockIdx.x != 0) continue;
    if (wave == 0) {
        if (mine) st->lane_iter[lane] = it;
        const int64_t b = tile * LDPC_WAVE + lane;
        if (over && b < (a.bp.rows_dev ? (int64_t)a.bp.rows_dev[0] : a.bp.batch)) {
            const int64_t row = a.bp.row_map ? (int64_t)a.bp.row_map[b] : b;
            const bool cv = ((ndone >> lane) & 1ull) != 0;
            if (a.bp.iters) a.bp.iters[row] = cv ? (mine ? it : st->lane_iter[lane]) : a.bp.max_iter;  // bp.hpp:304
            if (a.bp.conv) a.bp.conv[row] = cv ? 1 : 0;
        }
    }
    if (threadIdx.x == 0) {
        st->done[par ^ 1] = ndone;
        st->unsat[par ^ 1] = 0ull;
        st->llr_each[par ^ 1] = (each || newly) ? 1 : 0;  // after the first event: every bit pass stores the live lanes' posteriors
        if (over) {
            st->end_round = a.round;
            if (atomicSub(&a.bp.counters[2], 1u) == 1u && a.host_flag)  // that was the last live tile
                __hip_atomic_store(a.host_flag, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    } while (LOOP && (slot += (int)gridDim.y) < spread_count(a));
}

template <bool LOOP = false, bool RP = false>
__global__ void __launch_bounds__(256) bp_spread_finish_kernel(const SpreadArgs a) { spread_finish<LOOP, RP, false>(a); }

__global__ void __launch_bounds__(256) bp_spread_mem_finish_kernel(const SpreadArgs a) { spread_finish<false, false, true>(a); }

// ---- Relay-BP, the per-pass leg loop (host_stream.h: decode_relay): the per-row bookkeeping after each leg ----
// What a leg of the per-pass loop leaves per row, and what the loop keeps per row between legs.
struct RelaySelectArgs {
    int64_t batch;
    int32_t n, stop_after;
    int32_t first, last;            // this is leg 0 (the state starts here) / the last leg
    const double *llr0;             // [n]
    const uint8_t *leg_dec;         // [batch][n] the leg's decisions ...
    const double *leg_llr;          // [batch][n] ... posteriors (a converged row's: frozen at its convergence iteration) ...
    const int32_t *leg_iters;       // [batch]    ... iterations run ...
    const uint8_t *leg_conv;        // [batch]    ... and whether it reproduced the syndrome
    double *best_w;                 // [batch] the weight of the lightest solution so far (+inf: none)
    int32_t *nsol, *total;          // [batch] solutions so far; iterations so far
    uint8_t *decoding;              // the caller's outputs: [batch][n]
    double *llr;                    // [batch][n] or nullptr
    int32_t *iters;                 // [batch] or nullptr
    uint8_t *conv;                  // [batch] or nullptr
};

// One wavefront per row, after each leg: a row with stop_after solutions is finished and ignored; otherwise the leg's iterations are added, a
// solution is counted and -- if strictly lighter than the lightest so far (NaN never is) -- copied to the caller's outputs; a row without any
// solution gets the last leg's outputs.
__global__ void __launch_bounds__(256) relay_select_kernel(const RelaySelectArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= a.batch) return;
    double best = a.first ? __builtin_inf() : a.best_w[b];
    int nsol = a.first ? 0 : a.nsol[b], total = a.first ? 0 : a.total[b];
    if (nsol < a.stop_after) {
        total += a.leg_iters[b];
        const uint8_t *dec = a.leg_dec + b * a.n;
        bool take = false;
        if (a.leg_conv[b]) {
            const double w = relay_weight(a.llr0, a.n, lane, [&](int j) { return dec[j] != 0; });
            ++nsol;
            if (w < best) { best = w; take = true; }
        } else if (a.last && nsol == 0) {
            take = true;
        }
        if (take) {
            const double *src = a.leg_llr + b * a.n;
            for (int j = lane; j < a.n; j += LDPC_WAVE) {
                a.decoding[b * a.n + j] = dec[j];
                if (a.llr) a.llr[b * a.n + j] = src[j];
            }
        }
    }
    if (lane == 0) {
        a.best_w[b] = best;
        a.nsol[b] = nsol;
        a.total[b] = total;
        if (a.iters) a.iters[b] = total;
        if (a.conv) a.conv[b] = nsol > 0 ? 1 : 0;
    }
}
