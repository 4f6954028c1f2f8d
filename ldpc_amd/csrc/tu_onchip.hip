// tu_onchip.hip -- libldpc_hip.so, translation unit of the kernels that keep a syndrome's messages on chip (bp_small_kernel,
// bp_wave_kernel, bp_wave_ps_kernel, bp_edge_kernel, bp_edge8_kernel), with their host side (host_onchip.h: plans, tables, decode_onchip, and
// decode_onchip_f32 -- the host side of the FP32 lane = edge kernels, which tu_onchip_f32.hip instantiates; the row-prior lane = edge kernels
// are tu_onchip_rp.hip's).
#include "bp_device_common.h"
#include "bp_small_kernel.h"
#include "bp_wave_kernel.h"
#include "bp_edge_kernel.h"
#include "bp_edge_f32_kernel.h"  // (argument blocks and the kernel getters only: the FP32 instantiations are tu_onchip_f32.hip's)
#include "bp_edge_rp_kernel.h"   // (likewise: the row-prior instantiations are tu_onchip_rp.hip's)
#include "bp_edge_mem_kernel.h"  // (likewise: the memory instantiations are tu_onchip_mem.hip's)
#include "bp_edge_relay_kernel.h"  // (likewise: the Relay-BP instantiations are tu_onchip_relay.hip's)
#include "bp_wave_relay_kernel.h"  // (likewise: tu_onchip_wave_relay.hip's)
#include "bp_edge_gd_kernel.h"  // (likewise: the guided-decimation instantiations are tu_onchip_gd.hip's)
#include "bp_wave_gd_kernel.h"  // (likewise: tu_onchip_wave_gd.hip's)
#include "bp_wave_rp_kernel.h"  // (likewise: the row-prior lane = node instantiations are tu_onchip_wave_rp.hip's)
#include "bp_wave_f32_kernel.h"  // (likewise: the FP32 lane = node instantiations are tu_onchip_wave_f32.hip's)
#include "io_kernels.h"

#include "host_handle.h"
#include "host_onchip.h"
