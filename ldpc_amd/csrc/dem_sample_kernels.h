// dem_sample_kernels.h -- sampling a detector error model on the device, and counting the rows in which two bit-packed arrays differ
// Part of libldpc_hip.so: included by tu_dem.hip alone (host side: host_dem.h).  The specification is the NumPy twin
// ldpc_amd.noise_models.generate_dem_batch; the device reproduces it bit for bit.
//
//   e[b][j] = ((sm64(seed, (shot0 + b) * n + j) >> 11) < T[j])        the index convention of gen_bsc_errors_kernel, per-column thresholds
//   dets[b] = H e[b] mod 2,  obs[b] = L e[b] mod 2                    b8 rows: bit i of a shot is bit i % 8 of byte i / 8, padding bits 0
//
// One hash per (shot, column) -- not one per entry of H as in gen_bsc_syndromes_kernel -- and, errors being rare, sparse work after it: only the
// columns that fired touch their detectors.
#pragma once

#include "bp_device_common.h"

constexpr int DEM_WAVES = 4;  // wavefronts per workgroup, one shot each at a time
// 64 KiB of LDS a workgroup: what one wavefront gets for its two strips, in 32-bit words (ceil(m / 32) + ceil(k / 32) must fit)
constexpr int DEM_LDS_WORDS_PER_WAVE = 64 * 1024 / 4 / DEM_WAVES;

struct DemSampleArgs {
    const int32_t *col_ptr, *csc_row;          // columns of H: column j's detectors at [col_ptr[j], col_ptr[j + 1])
    const int32_t *obs_col_ptr, *obs_csc_row;  // columns of L (read only when obs != nullptr)
    const uint64_t *thr;                       // [n] thresholds
    int32_t m, n, k;
    uint64_t seed;
    int64_t shot0, batch;
    uint8_t *dets, *obs, *errs;                // [batch][ceil(m/8)], [batch][ceil(k/8)] or nullptr, [batch][ceil(n/8)] or nullptr
};

namespace dem {
// LDS operations of one wavefront execute in order; this pins the compiler and re-converges the lanes (as rel_lds::lds_sync)
__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bytes [off, off + 4) of a strip of little-endian words; off + 3 lies inside the strip
__device__ __forceinline__ uint32_t strip_dword(const uint32_t *words, int off) {
    const int w = off >> 2, sh = (off & 3) * 8;
    uint32_t v = words[w] >> sh;
    if (sh) v |= words[w + 1] << (32 - sh);
    return v;
}
__device__ __forceinline__ uint8_t strip_byte(const uint32_t *words, int off) { return (uint8_t)(words[off >> 2] >> ((off & 3) * 8)); }

// the wavefront writes bytes [0, nbytes) of a strip to dst, which starts on any byte: single bytes up to the first 4-byte boundary of dst,
// dwords from there, single bytes for what is left (fewer than 4)
__device__ __forceinline__ void store_strip(uint8_t *dst, const uint32_t *words, int nbytes, int lane) {
    int head = (int)((4u - (unsigned)((uintptr_t)dst & 3u)) & 3u);
    if (head > nbytes) head = nbytes;
    if (lane < head) dst[lane] = strip_byte(words, lane);
    const int body = (nbytes - head) >> 2;
    uint32_t *dst4 = (uint32_t *)(dst + head);
    for (int w = lane; w < body; w += 64) dst4[w] = strip_dword(words, head + 4 * w);
    const int done = head + 4 * body;
    if (lane < nbytes - done) dst[done + lane] = strip_byte(words, done + lane);
}
}  // namespace dem

// One wavefront per shot, workgroups of DEM_WAVES, every wavefront looping over shots b, b + DEM_WAVES * gridDim.x, ... (the host caps the grid).
// Lane l of step s draws column 64 s + l; the ballot of the 64 draws IS bytes 8 s .. 8 s + 7 of the shot's error row.  A lane that fired XORs its
// column's detectors / observables into the wavefront's own LDS strips (ceil(m / 32) and ceil(k / 32) words, cleared before the shot) with LDS
// atomics; the strips are the shot's b8 rows.  No workgroup barrier anywhere: the wavefronts of a workgroup share nothing.
// Dynamic LDS: DEM_WAVES * (ceil(m / 32) + ceil(k / 32)) words (k counted only with a.obs).
__global__ void __launch_bounds__(DEM_WAVES * 64) dem_sample_b8_kernel(const DemSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dem_lds[];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int mw = (a.m + 31) >> 5, kw = a.obs ? (a.k + 31) >> 5 : 0;
    uint32_t *det = dem_lds + (size_t)wave * (size_t)(mw + kw), *obs = det + mw;
    const int mb = (a.m + 7) >> 3, kb = (a.k + 7) >> 3, nb = (a.n + 7) >> 3;
    const int steps = (a.n + 63) >> 6;
    for (int64_t b = (int64_t)blockIdx.x * DEM_WAVES + wave; b < a.batch; b += (int64_t)gridDim.x * DEM_WAVES) {
        for (int w = lane; w < mw + kw; w += 64) det[w] = 0u;
        dem::lds_sync();
        const uint64_t base = (uint64_t)(a.shot0 + b) * (uint64_t)a.n;
        for (int s = 0; s < steps; ++s) {
            const int j = 64 * s + lane;
            bool fire = false;
            if (j < a.n) fire = (sm64(a.seed, base + (uint64_t)j) >> 11) < a.thr[j];
            const uint64_t fired = __ballot(fire);
            if (a.errs && lane < 8 && 8 * s + lane < nb) a.errs[b * nb + 8 * s + lane] = (uint8_t)(fired >> (8 * lane));
            if (fire) {
                for (int q = a.col_ptr[j]; q < a.col_ptr[j + 1]; ++q) {
                    const int r = a.csc_row[q];
                    atomicXor(&det[r >> 5], 1u << (r & 31));
                }
                if (kw)
                    for (int q = a.obs_col_ptr[j]; q < a.obs_col_ptr[j + 1]; ++q) {
                        const int r = a.obs_csc_row[q];
                        atomicXor(&obs[r >> 5], 1u << (r & 31));
                    }
            }
        }
        dem::lds_sync();
        dem::store_strip(a.dets + b * mb, det, mb, lane);
        if (kw) dem::store_strip(a.obs + b * kb, obs, kb, lane);
        dem::lds_sync();  // (the strips are read out before the next shot clears them)
    }
}

// rows of a [batch][ceil(bits / 8)] array that differ from the same row of b in their first `bits` bits (padding bits are not looked at):
// lane = row, the wavefront's ballot, one atomic add of its population count into the 64-bit counter; flags[row] = 0 / 1 when asked for.
// b == nullptr: a row counts when it is not all zero -- and with `invert`, when it IS (the rows whose converge byte is 0).
__global__ void __launch_bounds__(256) mismatch_b8_kernel(const uint8_t *__restrict__ x, const uint8_t *__restrict__ y, int64_t batch, int bits,
                                                          int invert, unsigned long long *count, uint8_t *flags) {
    const int nb = (bits + 7) >> 3, lane = (int)(threadIdx.x & 63u);
    const uint8_t last = (bits & 7) ? (uint8_t)((1u << (bits & 7)) - 1u) : (uint8_t)0xff;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * 64; r0 < batch; r0 += waves * 64) {  // (wave-uniform bounds: every lane reaches the ballot)
        const int64_t r = r0 + lane;
        bool differ = false;
        if (r < batch) {
            uint8_t acc = 0;
            for (int q = 0; q < nb; ++q) {
                uint8_t d = x[r * nb + q];
                if (y) d ^= y[r * nb + q];
                if (q == nb - 1) d &= last;
                acc |= d;
            }
            differ = invert ? acc == 0 : acc != 0;
            if (flags) flags[r] = (uint8_t)differ;
        }
        const uint64_t mask = __ballot(differ);
        if (lane == 0 && mask) atomicAdd(count, (unsigned long long)__popcll(mask));
    }
}
