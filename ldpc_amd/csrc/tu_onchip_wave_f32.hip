// tu_onchip_wave_f32.hip -- libldpc_hip.so, translation unit of the lane = node kernel with FP32 messages (bp_wave_f32_kernel.h): the twelve
// instantiations of bp_wave_f32_kernel -- the six rungs of LDPC_WAVE_LADDER (host_onchip.h), each with one wavefront and with a team per
// syndrome --, the kernel that writes their padded priors, and the functions that hand both to the host side in tu_onchip.hip (decode_wave_f32).
#include "bp_device_common.h"
#include "bp_wave_f32_kernel.h"

// the priors as the kernel reads them: llr0 rounded once to FP32 (v_cvt_f32_f64), 1.0f for the padding columns, FLT_MAX at np (a row's phantom entries)
__global__ void wave_f32_prior_pad_kernel(const double *llr0, int n, int np, float *out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < np + 2) out[q] = q < n ? (float)llr0[q] : q == np ? FLT_MAX : 1.0f;
}

WaveF32PriorKernel wave_f32_prior_kernel() { return wave_f32_prior_pad_kernel; }

WaveF32Kernel wave_f32_kernel(int dr, int dc, bool team) {
#define LDPC_WF(R, C) if (dr == R && dc == C) return team ? bp_wave_f32_kernel<R, C, true> : bp_wave_f32_kernel<R, C, false>;
    LDPC_WF(4, 2) LDPC_WF(4, 4) LDPC_WF(6, 3) LDPC_WF(8, 4) LDPC_WF(8, 8) LDPC_WF(16, 8)
#undef LDPC_WF
    return nullptr;
}
