// tu_onchip_relay.hip -- libldpc_hip.so, translation unit of the lane = edge Relay-BP kernels (bp_edge_relay_kernel.h): the 16
// instantiations of bp_edge_relay_kernel and the 18 of bp_edge8_relay_kernel -- the ladders of plan_edge and plan_edge8 (host_onchip.h) --
// and the two functions that hand them to the host side in tu_onchip.hip (decode_onchip_relay).
#include "bp_device_common.h"
#include "bp_edge_relay_kernel.h"

EdgeRelayKernel edge_relay_kernel(int rounds) {
    static const EdgeRelayKernel kerns[17] = {nullptr, bp_edge_relay_kernel<1>, bp_edge_relay_kernel<2>, bp_edge_relay_kernel<3>, bp_edge_relay_kernel<4>,
        bp_edge_relay_kernel<5>, bp_edge_relay_kernel<6>, bp_edge_relay_kernel<7>, bp_edge_relay_kernel<8>, bp_edge_relay_kernel<9>, bp_edge_relay_kernel<10>,
        bp_edge_relay_kernel<11>, bp_edge_relay_kernel<12>, bp_edge_relay_kernel<13>, bp_edge_relay_kernel<14>, bp_edge_relay_kernel<15>, bp_edge_relay_kernel<16>};
    return rounds < 1 || rounds > 16 ? nullptr : kerns[rounds];
}

Edge8RelayKernel edge8_relay_kernel(int rounds, int dc) {
#define LDPC_E8(R, C) if (rounds == R && dc == C) return bp_edge8_relay_kernel<R, C>;
    LDPC_E8(2, 3) LDPC_E8(3, 3) LDPC_E8(4, 3) LDPC_E8(5, 3) LDPC_E8(6, 3) LDPC_E8(7, 3) LDPC_E8(8, 3) LDPC_E8(9, 3) LDPC_E8(10, 3) LDPC_E8(12, 3)
    LDPC_E8(2, 4) LDPC_E8(3, 4) LDPC_E8(4, 4) LDPC_E8(5, 4) LDPC_E8(6, 4) LDPC_E8(7, 4) LDPC_E8(8, 4) LDPC_E8(9, 4)
#undef LDPC_E8
    return nullptr;
}
