// tu_dem.hip -- libldpc_hip.so, translation unit of the detector-error-model sampler: dem_sample_b8_kernel and mismatch_b8_kernel
// (dem_sample_kernels.h) with their host side (host_dem.h: ldpc_hip_bp_set_sampler, ldpc_hip_bp_sample_b8, ldpc_hip_count_mismatch_b8,
// ldpc_hip_bp_simulate_b8).  See bp_hip.hip for the design notes and the list of kernel headers.
#include "bp_device_common.h"
#include "dem_sample_kernels.h"
#include "io_kernels.h"

#include "host_handle.h"
#include "host_dem.h"
