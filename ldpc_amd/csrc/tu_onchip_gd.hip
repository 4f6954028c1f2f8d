// tu_onchip_gd.hip -- libldpc_hip.so, translation unit of the lane = edge guided-decimation kernels (bp_edge_gd_kernel.h): the 16
// instantiations of bp_edge_gd_kernel and the 18 of bp_edge8_gd_kernel -- the ladders LDPC_EDGE_LADDER and LDPC_EDGE8_LADDER (bp_edge_kernel.h), from which plan_edge and plan_edge8 (host_onchip.h) pick --
// and the two functions that hand them to the host side in tu_onchip.hip (decode_onchip_gd).
#include "bp_device_common.h"
#include "bp_edge_gd_kernel.h"

EdgeGdKernel edge_gd_kernel(int rounds) {
#define LDPC_E4(R) bp_edge_gd_kernel<R>,
    static const EdgeGdKernel kerns[17] = {nullptr, LDPC_EDGE_LADDER(LDPC_E4)};
#undef LDPC_E4
    return rounds < 1 || rounds > 16 ? nullptr : kerns[rounds];
}

Edge8GdKernel edge8_gd_kernel(int rounds, int dc) {
#define LDPC_E8(R, C) if (rounds == R && dc == C) return bp_edge8_gd_kernel<R, C>;
    LDPC_EDGE8_LADDER(LDPC_E8)
#undef LDPC_E8
    return nullptr;
}
