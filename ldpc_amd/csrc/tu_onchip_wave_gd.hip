// tu_onchip_wave_gd.hip -- libldpc_hip.so, translation unit of the lane = node guided-decimation kernel (bp_wave_gd_kernel.h): the twelve
// instantiations of bp_wave_gd_kernel -- the six rungs of pick_wave (host_onchip.h), each with one wavefront and with a team per syndrome --
// and the function that hands them to the host side in tu_onchip.hip (decode_wave_gd).
#include "bp_device_common.h"
#include "bp_wave_gd_kernel.h"

WaveGdKernel wave_gd_kernel(int dr, int dc, bool team) {
#define LDPC_WG(R, C) if (dr == R && dc == C) return team ? bp_wave_gd_kernel<R, C, true> : bp_wave_gd_kernel<R, C, false>;
    LDPC_WG(4, 2) LDPC_WG(4, 4) LDPC_WG(6, 3) LDPC_WG(8, 4) LDPC_WG(8, 8) LDPC_WG(16, 8)
#undef LDPC_WG
    return nullptr;
}
