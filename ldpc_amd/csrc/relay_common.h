// relay_common.h -- what the routes of Relay-BP (ldpc_hip_bp_set_relay) share on the device: the weight of a solution
// Part of libldpc_hip.so: included by bp_edge_relay_kernel.h (tu_onchip_relay.hip), bp_wave_relay_kernel.h (tu_onchip_wave_relay.hip) and bp_spread_kernels.h (tu_stream.hip: relay_select_kernel).
#pragma once

#include "bp_device_common.h"

// The weight of a row's decisions, sum over the decided bits of their prior log-ratios, as an FP64 sum in ONE fixed order -- so that the lane =
// edge kernels, bp_wave_relay_kernel, relay_select_kernel and the NumPy restatement (tests/relay_bp_util.py: relay_weight) form the same bits:
//     t[j] = dec[j] ? L0[j] : +0.0                                  (a select, never a product)
//     p[lane] = ((0.0 + t[lane]) + t[lane + 64]) + ...              over j < n ascending, lane = 0 .. 63
//     p[lane] = p[lane] + p[lane ^ s]  for s = 1, 2, 4, 8, 16, 32   (an addition commutes: both lanes of a pair hold the same bits)
// Every lane returns the weight.  `one(j)`: is bit j decided 1; the whole wavefront calls this together.
template <class ONE>
__device__ __forceinline__ double relay_weight(const double *__restrict__ llr0, int n, int lane, ONE one) {
    double p = 0.0;
    for (int j = lane; j < n; j += LDPC_WAVE) p = p + (one(j) ? llr0[j] : 0.0);
#pragma unroll
    for (int s = 1; s < LDPC_WAVE; s <<= 1) p = p + __shfl_xor(p, s, LDPC_WAVE);
    return p;
}
