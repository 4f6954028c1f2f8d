// tu_onchip_wave_rp.hip -- libldpc_hip.so, translation unit of the lane = node row-prior kernel (bp_wave_rp_kernel.h): the twelve
// instantiations of bp_wave_rp_kernel -- the six rungs of pick_wave (host_onchip.h), each with one wavefront and with a team per syndrome --
// and the function that hands them to the host side in tu_onchip.hip (decode_wave_rp).
#include "bp_device_common.h"
#include "bp_wave_rp_kernel.h"

WaveRpKernel wave_rp_kernel(int dr, int dc, bool team) {
#define LDPC_WR(R, C) if (dr == R && dc == C) return team ? bp_wave_rp_kernel<R, C, true> : bp_wave_rp_kernel<R, C, false>;
    LDPC_WR(4, 2) LDPC_WR(4, 4) LDPC_WR(6, 3) LDPC_WR(8, 4) LDPC_WR(8, 8) LDPC_WR(16, 8)
#undef LDPC_WR
    return nullptr;
}
