// tu_onchip_f32.hip -- libldpc_hip.so, translation unit of the lane = edge kernels with FP32 messages (bp_edge_f32_kernel.h): the 84
// instantiations of bp_edge_f32_kernel and bp_edge8_f32_kernel -- the ladders of plan_edge and plan_edge8 (host_onchip.h) -- and the two
// functions that hand them to the host side in tu_onchip.hip (decode_onchip_f32).
#include "bp_device_common.h"
#include "bp_edge_f32_kernel.h"

EdgeF32Kernel edge_f32_kernel(int rounds, bool uniform, bool noclamp) {
#define LDPC_EDGE_ROW(...) {nullptr, bp_edge_f32_kernel<1, __VA_ARGS__>, bp_edge_f32_kernel<2, __VA_ARGS__>, bp_edge_f32_kernel<3, __VA_ARGS__>, \
        bp_edge_f32_kernel<4, __VA_ARGS__>, bp_edge_f32_kernel<5, __VA_ARGS__>, bp_edge_f32_kernel<6, __VA_ARGS__>, bp_edge_f32_kernel<7, __VA_ARGS__>, \
        bp_edge_f32_kernel<8, __VA_ARGS__>, bp_edge_f32_kernel<9, __VA_ARGS__>, bp_edge_f32_kernel<10, __VA_ARGS__>, bp_edge_f32_kernel<11, __VA_ARGS__>, \
        bp_edge_f32_kernel<12, __VA_ARGS__>, bp_edge_f32_kernel<13, __VA_ARGS__>, bp_edge_f32_kernel<14, __VA_ARGS__>, bp_edge_f32_kernel<15, __VA_ARGS__>, \
        bp_edge_f32_kernel<16, __VA_ARGS__>}
    static const EdgeF32Kernel kerns[3][17] = {LDPC_EDGE_ROW(false), LDPC_EDGE_ROW(true), LDPC_EDGE_ROW(true, true)};
#undef LDPC_EDGE_ROW
    if (rounds < 1 || rounds > 16 || (noclamp && !uniform)) return nullptr;
    return kerns[uniform ? (noclamp ? 2 : 1) : 0][rounds];
}

Edge8F32Kernel edge8_f32_kernel(int rounds, int dc, bool uniform) {
#define LDPC_E8(R, C) if (rounds == R && dc == C) return uniform ? bp_edge8_f32_kernel<R, C, true> : bp_edge8_f32_kernel<R, C, false>;
    LDPC_E8(2, 3) LDPC_E8(3, 3) LDPC_E8(4, 3) LDPC_E8(5, 3) LDPC_E8(6, 3) LDPC_E8(7, 3) LDPC_E8(8, 3) LDPC_E8(9, 3) LDPC_E8(10, 3) LDPC_E8(12, 3)
    LDPC_E8(2, 4) LDPC_E8(3, 4) LDPC_E8(4, 4) LDPC_E8(5, 4) LDPC_E8(6, 4) LDPC_E8(7, 4) LDPC_E8(8, 4) LDPC_E8(9, 4)
#undef LDPC_E8
    return nullptr;
}
