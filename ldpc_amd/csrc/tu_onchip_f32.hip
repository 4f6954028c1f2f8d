// tu_onchip_f32.hip -- libldpc_hip.so, translation unit of the lane = edge kernels with FP32 messages (bp_edge_f32_kernel.h): the 84
// instantiations of bp_edge_f32_kernel and bp_edge8_f32_kernel -- the ladders LDPC_EDGE_LADDER and LDPC_EDGE8_LADDER (bp_edge_kernel.h), from which plan_edge and plan_edge8 (host_onchip.h) pick -- and the two
// functions that hand them to the host side in tu_onchip.hip (decode_onchip_f32).
#include "bp_device_common.h"
#include "bp_edge_f32_kernel.h"

EdgeF32Kernel edge_f32_kernel(int rounds, bool uniform, bool noclamp) {
#define LDPC_GENERAL(R) bp_edge_f32_kernel<R, false>,
#define LDPC_UNIFORM(R) bp_edge_f32_kernel<R, true>,
#define LDPC_NOCLAMP(R) bp_edge_f32_kernel<R, true, true>,
    static const EdgeF32Kernel kerns[3][17] = {{nullptr, LDPC_EDGE_LADDER(LDPC_GENERAL)}, {nullptr, LDPC_EDGE_LADDER(LDPC_UNIFORM)}, {nullptr, LDPC_EDGE_LADDER(LDPC_NOCLAMP)}};
#undef LDPC_GENERAL
#undef LDPC_UNIFORM
#undef LDPC_NOCLAMP
    if (rounds < 1 || rounds > 16 || (noclamp && !uniform)) return nullptr;
    return kerns[uniform ? (noclamp ? 2 : 1) : 0][rounds];
}

Edge8F32Kernel edge8_f32_kernel(int rounds, int dc, bool uniform) {
#define LDPC_E8(R, C) if (rounds == R && dc == C) return uniform ? bp_edge8_f32_kernel<R, C, true> : bp_edge8_f32_kernel<R, C, false>;
    LDPC_EDGE8_LADDER(LDPC_E8)
#undef LDPC_E8
    return nullptr;
}
