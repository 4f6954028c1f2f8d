// tu_f32.hip -- libldpc_hip.so, translation unit of the float32 message mode: the per-pass min-sum kernels bp_f32_* (bp_f32_kernels.h)
// with their host side (host_f32.h: decode_f32).  See bp_hip.hip for the design notes and the list of kernel headers.
#include "bp_device_common.h"
#include "bp_f32_kernels.h"
#include "io_kernels.h"

#include "host_handle.h"
#include "host_f32.h"
