// host_handle.h -- the handle (struct ldpc_hip_bp), error reporting, device buffers, measurement switches
// Part of libldpc_hip.so: included by every translation unit (bp_hip.hip = the C ABI; tu_stream / tu_serial / tu_onchip / tu_onchip_f32 / tu_onchip_rp / tu_onchip_mem / tu_onchip_relay / tu_onchip_wave_relay / tu_onchip_gd / tu_onchip_wave_gd / tu_onchip_wave_f32 / tu_osd / tu_f32.hip = one kernel
// family each with its host side).  What one unit calls in another is declared at the end of this header.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <random>
#include <atomic>
#include <thread>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>

#include <cxxabi.h>
#include <unistd.h>

#include <sys/mman.h>

#include "mem_host.h"
#include "mode_host.h"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

inline thread_local std::string g_last_error;  // (one per thread for the whole library: C++17 inline variable)

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(_e == hipErrorOutOfMemory ? LDPC_HIP_ERR_NOMEM : LDPC_HIP_ERR_DEVICE, \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,      \
                        __LINE__);                                                            \
    } while (0)

inline std::atomic<long long> g_device_buf_bytes{0};  // bytes every live DeviceBuf of the process holds (ldpc_hip_debug_device_buf_bytes)

// Launch log (ldpc_hip_debug_launch_log / ldpc_hip_debug_launch_log_read, LDPC_HIP_LAUNCH_LOG=<file>): which kernel instantiations the process
// launched, name -> count.  EVERY launch of the library goes through LDPC_LAUNCH / LDPC_LAUNCH_TIMED / LDPC_LAUNCH_PTR below (tests/test_layout.py
// looks for strays), which hand the launched host-function pointer to launch_log_note when the log is on; off, a launch costs one load of the flag.
// A pointer's name is resolved once, when it is first recorded: the runtime's name of the kernel (hipKernelNameRefByPtr -- it names every kernel
// of the library, those with internal linkage in several translation units included), demangled and cut to the spelling of
// tools/list_instantiations.py -- "bp_edge8_kernel<12, 3, true>"; "?<pointer>" should it ever know none (the tests that read the log then fail).
inline std::atomic<bool> g_launch_log_on{false};
struct LaunchLog {
    std::mutex mu;  // (the host pipeline and multi_device.h launch from several threads)
    std::unordered_map<const void *, std::string> names;
    std::map<std::string, long long> counts;  // since ldpc_hip_debug_launch_log(1)
    std::map<std::string, long long> total;   // of the process, kept only for LDPC_HIP_LAUNCH_LOG=<file>: the calls above do not clear it
    bool by_call = false;
    std::string file;                         // empty: no LDPC_HIP_LAUNCH_LOG
};
inline LaunchLog &launch_log() {
    static LaunchLog *const log = new LaunchLog;  // never destroyed: the table is written out while the library unloads (host_setup.h)
    return *log;
}

inline std::string launch_log_spelling(const char *mangled) {
    std::string s = mangled;
    if (s.size() > 3 && s.compare(s.size() - 3, 3, ".kd") == 0) s.resize(s.size() - 3);
    int status = -1;
    char *d = abi::__cxa_demangle(s.c_str(), nullptr, nullptr, &status);
    if ((status != 0 || !d) && s.find('.') != std::string::npos) {  // (a kernel with internal linkage may carry a ".suffix" of its translation unit)
        std::free(d);
        d = abi::__cxa_demangle(s.substr(0, s.find('.')).c_str(), nullptr, nullptr, &status);
    }
    if (status == 0 && d) s = d;
    std::free(d);
    for (size_t at; (at = s.find("void ")) != std::string::npos;) s.erase(at, 5);
    if (s.find('(') != std::string::npos) s.resize(s.find('('));
    while (!s.empty() && s.back() == ' ') s.pop_back();
    return s;
}

inline void launch_log_note(const void *host_fn, hipStream_t stream) {
    LaunchLog &log = launch_log();
    std::lock_guard<std::mutex> lock(log.mu);
    auto it = log.names.find(host_fn);
    if (it == log.names.end()) {
        const char *ref = hipKernelNameRefByPtr(host_fn, stream);
        std::string name = ref && *ref ? launch_log_spelling(ref) : std::string();
        if (name.empty()) {
            char buf[32];
            snprintf(buf, sizeof buf, "?%p", host_fn);
            name = buf;
        }
        it = log.names.emplace(host_fn, std::move(name)).first;
    }
    if (log.by_call) ++log.counts[it->second];
    if (!log.file.empty()) ++log.total[it->second];
}

// `kern`: a kernel's name -- a template-id in its own parentheses, (bp_edge0_kernel<M, F>) -- or a pointer a plan picked
#define LDPC_LAUNCH(kern, grid, block, dyn, stream, ...)                                                      \
    do {                                                                                                      \
        if (g_launch_log_on.load(std::memory_order_relaxed)) launch_log_note((const void *)(kern), (stream)); \
        hipLaunchKernelGGL(kern, grid, block, dyn, stream, __VA_ARGS__);                                      \
    } while (0)
// ... with the timing events on the dispatch itself (hipExtLaunchKernelGGL)
#define LDPC_LAUNCH_TIMED(kern, grid, block, dyn, stream, ev_start, ev_stop, flags, ...)                      \
    do {                                                                                                      \
        if (g_launch_log_on.load(std::memory_order_relaxed)) launch_log_note((const void *)(kern), (stream)); \
        hipExtLaunchKernelGGL(kern, grid, block, dyn, stream, ev_start, ev_stop, flags, __VA_ARGS__);         \
    } while (0)
// ... with the arguments as an array of pointers (hipLaunchKernel); an expression: the launch's hipError_t
#define LDPC_LAUNCH_PTR(fn, grid, block, params, dyn, stream) \
    ((g_launch_log_on.load(std::memory_order_relaxed) ? launch_log_note((const void *)(fn), (stream)) : (void)0), hipLaunchKernel((fn), grid, block, params, dyn, stream))

struct DeviceBuf {  // grow-only device allocation, freed with its owner (on the device that is current then: see ldpc_hip_bp_destroy)
    void *p = nullptr;
    size_t cap = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }  // (std::vector<MultiDev>)
    ~DeviceBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(LDPC_HIP_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes,
                        hipGetErrorString(e));
        }
        cap = bytes;
        g_device_buf_bytes += (long long)bytes;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        g_device_buf_bytes -= (long long)cap;
        p = nullptr;
        cap = 0;
    }
};

// Measurement / test switches (none changes a result; profiles/README.md lists them).  They live in the handle: seeded ONCE, at
// creation, from the environment variables LDPC_HIP_<NAME>, changed afterwards only through ldpc_hip_bp_set_debug_switch -- no
// getenv on the decode path, and nothing a test can change under a live handle by accident.
static const char *const k_switch_names[] = {"PS_TEAM", "EXPLICIT_INIT", "OSD_UNBLOCKED", "OSD_PLANES",
                                             "PS_TEAM_WAVES", "EDGE_STATIC_PCT", "EDGE_CHUNK", "NO_HOST_PIPELINE", "NO_DIRECT_LLR", "HOST_CHUNK_ROWS", "TIME_SMALL_CALLS", "REL_LDS", "HOST_PIPE_TIMING", "REL_LEVELS", "REL_PROF", "REL_SCRATCH_IN_L", "SER_RING", "SER_WAVES", "SER_LANE_MAX", "SER_LANE_THREADS", "SER_WAVES2", "RESIDENT", "SER_NO_REMAINDER", "SER_ROUND_TILES", "VAR_RING", "VAR_RING_UNITS", "SPREAD_NODES", "SER_VAR", "SER_VAR_UNITS", "REL_EXT", "OSD_COLLECT_AFTER", "EDGE_CLAMP", "OSD_NO_FLAT", "F32_NT", "F32_GRID_ROWS", "F32_ONCHIP", "F32_REPACK_MIN_TILES", "EDGE_RP", "SPREAD_NT", "REPACK_MIN_TILES", "DEM_GRID", "F32_WAVE_LLR", "WAVE_RP"};
constexpr int k_n_switches = (int)(sizeof(k_switch_names) / sizeof(k_switch_names[0]));

struct ldpc_hip_bp {
    int32_t switches[k_n_switches];  // -1 = not set
    int sw(const char *name) const {  // value of a switch, -1 when it is not set
        for (int i = 0; i < k_n_switches; ++i)
            if (!std::strcmp(name, k_switch_names[i])) return switches[i];
        return -1;
    }
    bool on(const char *name) const { return sw(name) > 0; }
    int device = 0;
    int32_t m = 0, n = 0, nnz = 0;
    int32_t max_iter = 1, bp_method = 0;
    double ms_scaling_factor = 1.0;
    int32_t max_row_deg = 0, max_col_deg = 0;
    int32_t waves_per_wg = 0;  // 0 = auto
    int32_t math_mode = LDPC_HIP_MATH_LIBM_EXACT;
    int32_t msg_dtype = LDPC_HIP_MSG_F64;  // ldpc_hip_bp_set_message_dtype: LDPC_HIP_MSG_F32 routes decode_device to decode_f32 (tu_f32.hip)
    DeviceBuf f32_llr0;      // ... [n] the priors rounded to FP32
    bool f32_lane_node = false;  // ldpc_hip_bp_set_f32_lane_node: float32 decodes of codes beyond both lane = edge ladders go to bp_wave_f32_kernel (opt-in; a handle setting like small_mode, read only by float32 decodes)
    DeviceBuf w_prior_f32;   // bp_wave_f32_kernel: [np + 2] the padded priors as floats (before every launch; released when the route is switched off)
    bool regular = false;   // every row has the same weight and every column has the same weight
    int32_t ring_depth = 2; // LDS-DMA ring slots per wavefront for regular matrices (0 = register variant)
    int32_t small_mode = -1; // on-chip kernels for small codes: -1 auto, 0 never, 1 whenever one fits, 2 the slot kernel only
    std::vector<int32_t> h_row_ptr, h_col_idx;  // host copy of the CSR arrays
    std::vector<int32_t> h_col_ptr, h_csc_edge, h_csc_row;  // ... and of the column view: column j's entries at [h_col_ptr[j], h_col_ptr[j + 1]), rows ascending, as CSR edge / row
    int wave_dr = 0, wave_dc = 0;  // template bounds the uploaded SoA position tables of bp_wave_kernel were built for (0: none)
    int wave_ps_dr = 0, wave_ps_dc = 0;  // likewise for bp_wave_ps_kernel
    DeviceBuf wp_rdeg, wp_col, wp_epos;
    DeviceBuf w_rdeg, w_cdeg, w_col, w_apos, w_prior;
    DeviceBuf d_edge0;       // [n] initial edge values of the streamed kernel (BpArgs::edge0)
    DeviceBuf var_row_items, var_pair_items;  // item tables of the variable-degree ring (BpArgs::row_items, pair_items; host_stream.h: ensure_var_ring_items)
    bool var_items_built = false;
    int edge_rounds = 0;     // rounds the uploaded slot tables of bp_edge_kernel were built for (0: none)
    DeviceBuf e_partner, e_kind, e_scol, e_prior;
    int32_t handoff = -1;    // straggler hand-off threshold in tiles: -1 auto (256), 0 off
    DeviceBuf tile_state, handoff_list;
    unsigned *h_counters = nullptr;  // pinned host copy of the device counters
    // Per-pass rounds are queued without waiting for the device.  The kernel that finalises the last running tile writes
    // the decode's sequence number into this host-mapped word; the host merely LOOKS at it before queueing the next round
    // (no synchronisation) and stops queueing once it matches -- rounds queued past that point find nothing to do.
    unsigned *h_flag = nullptr, *d_flag = nullptr;
    unsigned flag_seq = 0;
    unsigned long long *d_clk = nullptr;  // {shader cycles, constant-rate ticks} summed over the workgroups of the long-running BP kernels (clock_probe_*)
    int32_t schedule = 1;    // ldpc::bp::BpSchedule (bp.hpp:28-32): 0 serial, 1 parallel, 2 serial_relative
    // What the reference keeps in the decoder OBJECT from one decode to the next (bp.hpp:67, 75): serial_schedule_order -- the
    // arrangement serial_relative re-sorts and the random schedule re-shuffles every iteration -- and the generator of the shuffles.
    std::vector<int32_t> sched_state;
    std::mt19937 sched_rng;
    int32_t sched_seed_raw = 0;  // random_schedule_seed as given (the soft-syndrome routine seeds its own engine with it)
    bool random_serial = false;
    DeviceBuf rel_ord, rel_dbit, sched_orders, sched_order0;
    DeviceBuf sched_lvl_bits, sched_lvl_ptr;      // the random schedule's orders once more, level-major, and their level bounds (host_serial.h: random_orders_*)
    DeviceBuf rl_edge, rl_chk, rl_cdeg, rl_last;  // per-column tables and the last row's final order of bp_relative_lds_kernel
    int rl_dc = 0;                                // stride the tables were built for (0: none)
    DeviceBuf rl_first;                           // the order after the first iteration's sort of the current call (RelLdsArgs::first_order)
    DeviceBuf rl_rec, rl_ext_A;                   // EXT form: the per-entry records [n][dc] u64; the wavefronts' message slots [workgroups][wavefronts][nnz] f64
    bool rl_rec_valid = false;
    // The random schedule's table of per-iteration orders (host_serial.h: random_orders_*), kept on the device between calls as a
    // ring of max_iter rows: a call consumes as many rows as its LAST row ran iterations, and only those are generated anew.
    struct RandomOrders {
        bool valid = false;
        int kind = 0, rows = 0, n = 0, first = 0;   // kind 0: one std::mt19937 stream (bp.hpp:467-469); 1: a new default_random_engine(seed) per shuffle (bp.hpp:573-577)
        int32_t seed_raw = 0;
        std::mt19937 rng_end;                       // generator behind the table's last row (kind 0)
        std::vector<int> row_end;                   // the table's last row
        std::vector<int32_t> n_levels;              // levels of every row of the ring (0: row not built)
        std::vector<int32_t> expect_state;          // what the handle's order / generator must be for the table to be current
        std::mt19937 expect_rng;
    } rnd;
    int32_t *d_csc_row = nullptr, *d_order = nullptr;
    bool custom_order = false;
    DeviceBuf counter;  // counter_bytes(): the BP kernels' work pools, then the counters of BP + OSD (osd_counter_ptr)
    // BP + OSD: where an on-chip BP kernel that can do so lists the rows it leaves unconverged (bposd_device arms it around its decode_device call;
    // `done` says a kernel honoured it -- and then also zeroed the counters, which sit behind the work pools in `counter`)
    struct { int32_t *list; unsigned *count; uint8_t *status; bool armed, done; } osd_hook = {nullptr, nullptr, nullptr, false, false};
    std::vector<double> channel_probs;

    int32_t *d_row_ptr = nullptr, *d_col_idx = nullptr, *d_col_ptr = nullptr, *d_csc_edge = nullptr;
    double *d_llr0 = nullptr;
    double *d_osd_wt = nullptr;  // [n] log(1 / p_j), the candidate weights of higher-order OSD
    bool osd_reg = true;  // register-resident elimination for small matrices (ldpc_hip_bp_set_osd_kernel)
    bool osd_big = false; // OSD through osd_big_kernel whatever the size (testing)
    int osd_k_cached = -1;  // n - rank(H), computed on first use
    int32_t osd_method = 1, osd_order = 0;  // ldpc::osd::OsdMethod (osd.hpp:18-23) used by ldpc_hip_bposd_decode_batch

    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr;  // ev_mid: end of the persistent kernel, when one ran
    hipEvent_t evp0 = nullptr, evp1 = nullptr, evp_mid = nullptr;  // the same of the first pass of a two-pass decode (decode_stream_repacked)
    bool timed_prev = false, timed_prev_mid = false;
    hipEvent_t ev_done = nullptr;  // end of the last call that queued work on `stream` (orders a change of stream after it)
    bool work_queued = false;
    bool timed = false, timed_mid = false;
    bool untimed_call = false;  // a single decode() through the host-mapped block: the two timing events cost more than they tell (ldpc_hip_bp_last_kernel_ms then says 0)
    float accumulated_ms = 0.f, accumulated_persistent_ms = 0.f;

    DeviceBuf msgA, msgC, par, nzm, invalid, dec, dcur, llr_t;       // workspace
    DeviceBuf st_synd, st_dec, st_llr, st_iters, st_conv, st_misc;  // staging for host pointers
    // small calls with host buffers (a single decode()): one host-mapped, coherent block that the kernels read and write in place --
    // no copy commands at all, one launch sequence and one wait
    unsigned char *pin_host = nullptr, *pin_dev = nullptr;
    static constexpr size_t PIN_BYTES = 512u * 1024u;
    static constexpr size_t PIN_MAIL = PIN_BYTES - 64;  // the last 64 bytes: the resident kernel's mailbox (WavePsArgs::mail)
    // A single decode() of a small code (host buffers, product-sum, parallel schedule) is served by a RESIDENT workgroup that stays for
    // `linger` after its last request (host_onchip.h: decode_onchip_resident): no launch, no completion, tables already in LDS.
    struct Resident {
        hipStream_t stream = nullptr;
        hipEvent_t ended = nullptr;       // behind the resident kernel's launch: has it left?
        bool launched = false;            // a launch whose end has not been seen yet
        unsigned seq = 0;                 // the last request number handed out
        unsigned long long key[6] = {};   // what the kernel in flight was launched for (parameters, priors, plan): a change retires it
    } res;
    unsigned long long priors_version = 0;  // bumped whenever the priors on the device change (upload_priors)
    // large calls with host buffers: pinned double-buffered chunks, so that PCIe and the host's own copies overlap the kernels
    // (host_decode_abi.h: decode_batch_pipelined)
    struct HostPipe {
        static constexpr int NB = 3;  // chunks in flight: one being decoded, one on its way out over PCIe, one being copied into the caller's arrays
        hipStream_t s_in = nullptr, s_out = nullptr;
        hipEvent_t ev_in[NB] = {}, ev_cmp[NB] = {}, ev_out[NB] = {};
        unsigned char *pin_in[NB] = {}, *pin_out[NB] = {};
        size_t pin_in_cap = 0, pin_out_cap = 0;
        DeviceBuf d_in[NB], d_dec[NB], d_llr[NB], d_it[NB], d_cv[NB];
    } pipe;
    DeviceBuf osd_llr, osd_conv;                                    // BP outputs OSD-0 needs when the caller does not ask for them
    DeviceBuf osd_scratch;                                          // working copies of H for osd_big_kernel
    DeviceBuf osd_packed;                                           // [m][words] H bit-packed by rows (register OSD kernels)
    DeviceBuf osd_ell;                                              // [m][8] a row's entries as 16-bit column numbers (osd0_flat_kernel)
    DeviceBuf osd_list, osd_counters;                               // rows BP left unconverged + {count, next}
    DeviceBuf osd_status;                                           // [batch] of the last BP + OSD decode: 0 BP converged, 1 OSD solved, 2 s outside image(H)
    DeviceBuf osd_fix_synd, osd_fix_list, osd_fix_scratch;  // second OSD pass over the rows outside the image (osd_exact_kernel.h)
    int64_t osd_status_rows = 0;
    DeviceBuf rp_synd, rp_dec, rp_llr, rp_iters, rp_conv;           // repacked second pass of the serial schedule
    int32_t serial_kernel = -1;                                     // -1 auto, 0 one wavefront per tile, 1 level-parallel workgroup per tile
    bool order_visits_all = true;                                   // false: some bit is never updated (its outputs stay 0)
    bool levels_valid = false;                                      // lvl_* describe the current schedule order
    int32_t n_levels = 0;
    DeviceBuf lvl_ptr, lvl_bits;
    std::vector<int32_t> h_lvl_ptr, h_lvl_bits;                     // host copies (the streamed serial kernel's position records are built from them)
    DeviceBuf ser_pos_e0;                                            // ... and the initial values of every position's other entries (first iteration)
    DeviceBuf ser_rows[2], ser_synd2;                                // decode_serial_streamed: the rows of a compacted pass (numbers in the caller's arrays), their syndromes
    DeviceBuf ser_pos_tab;                                           // bp_serial_stream_kernel: one record per position of the level-major order
    bool ser_pos_valid = false;                                     // ... describing the current levels
    DeviceBuf ser_var_init;                                         // ... [nnz][64] initial segments shared by all tiles (SerialArgs::var_init), rewritten by every decode that uses it
    DeviceBuf ser_var_items, ser_var_wq, ser_var_lane_items, ser_var_lane_lvl;  // bp_serial_var_kernel.h: item streams per (level, wavefront); the level-major item list of the lane kernel
    bool ser_var_valid = false;                                     // ... describing the current levels, for ser_var_waves wavefronts per tile
    int ser_var_waves = 0;
    int32_t min_col_deg = 0;
    // repacking of the streamed parallel schedule (decode_stream_repacked), steered by what the previous decode looked like
    DeviceBuf sp_hist, sp_iters;     // iteration histogram of the last streamed decode (256 bins) / iteration counts when the caller wants none
    unsigned *h_hist = nullptr;      // pinned copy of the histogram
    hipEvent_t ev_hist = nullptr;    // the copy has landed
    bool hist_pending = false;
    int32_t hist_max_iter = 0;
    unsigned hist_landed[256] = {};  // the last histogram whose copy was SEEN complete (never waited for)
    bool hist_landed_valid = false;
    int32_t hist_landed_max_iter = 0;
    int32_t repack_iters = -1;                                      // first-pass iterations: -1 auto (stream_first_pass_length: the last histogram decides), 0 = no repacking
    DeviceBuf soft_S, soft_in, soft_out;                             // soft-syndrome decoding: scaled analog syndromes, staging
    DeviceBuf b8_in, b8_out, b8_synd, b8_dec, obs_row_ptr, obs_col_idx;  // bit-packed shot I/O and the observables matrix
    int32_t obs_k = -1;                                              // rows of the observables matrix (-1: not set)
    std::vector<int32_t> h_obs_row_ptr, h_obs_col_idx;               // host copy of the observables matrix (its column view is built from it: dem_upload_obs_csc)
    // Sampling of the detector error model (host_dem.h, tu_dem.hip): the per-column thresholds of ldpc_hip_bp_set_sampler -- independent of the
    // decoding priors -- the column view of the observables matrix, and what ldpc_hip_bp_simulate_b8 keeps on the device per chunk
    bool sampler_set = false;
    DeviceBuf dem_thr, dem_obs_col_ptr, dem_obs_csc_row;             // [n] u64; [n + 1], [nnz(L)]
    DeviceBuf sim_dets, sim_obs, sim_err, sim_pred, sim_conv, sim_count;  // a chunk's sampled rows, true and predicted observables, converge flags; the two 64-bit counters
    int64_t max_chunk_tiles = 0;                                     // 0 = decide from free memory
    // Row priors (ldpc_hip_*_decode_batch_priors): the call's [batch][n] channel probabilities on the device while it runs, nullptr
    // otherwise -- decode_device, the streamed decode (host_stream.h: rp) and decode_onchip look here, nobody else; the handle's own channel_probs / d_llr0 are not touched.
    const double *row_probs = nullptr;
    DeviceBuf rowp_llr;  // their log-ratios: in tile layout [tiles of a chunk][n][64] (io_kernels.h: row_priors_kernel), or row-major [batch][n] for the lane = edge kernels (row_priors_rowmajor_kernel), or padded rows [batch][np + 2] for the lane = node kernel (wave_rp_prior_kernel, host_onchip.h)
    DeviceBuf st_probs;  // staging for a host pointer
    // Which of memory min-sum, Relay-BP and guided decimation is on -- at most one: the three setters switch it and refuse a second (mode_host.h: mode_exclusion)
    Variant variant = Variant::Plain;
    // Memory min-sum BP (ldpc_hip_bp_set_memory): every iteration's bit pass takes a[j] + gamma[j] * (the column's previous
    // posterior) for the prior.  decode_device looks at `variant` and sends the batch to the memory kernels (bp_edge_mem_kernel.h, the bp_spread_mem_* kernels of
    // bp_spread_kernels.h); with it off nothing below is read.  The per-pass route keeps the posteriors M [tiles of a chunk][n][64] in rowp_llr
    // (row priors and memory exclude each other).
    std::vector<double> mem_gamma;  // [n] the strengths as given
    int mem_bad_col = -1;           // first column with gamma != 0 whose prior is not finite, for the priors the handle holds NOW (-1: none)
    DeviceBuf mem_ag;               // [2][n]: a[] = (1 - gamma) * log((1 - p) / p) (mem_host.h), then gamma[]; rewritten by upload_memory
    DeviceBuf e_mem;                // [2][R * 64]: a and gamma of every slot of the lane = edge tables (edge_mem_table_kernel, before every launch)
    // Relay-BP (ldpc_hip_bp_set_relay): relay_legs memory legs chained per syndrome -- leg l runs up to relay_iters[l] iterations
    // with the strengths relay_gamma[l][.] and starts from the posteriors the leg before it ended with; the lightest of the first relay_stop
    // solutions is the result.  decode_device looks at `variant` and sends the batch to decode_relay (host_stream.h): the lane = edge relay kernels
    // (bp_edge_relay_kernel.h), the lane = node kernel (bp_wave_relay_kernel.h), or a loop of per-pass memory decodes with relay_select_kernel after each.  Relay and memory exclude each other.
    int32_t relay_legs = 0, relay_stop = 0;
    std::vector<double> relay_gamma;    // [legs][n] the strengths as given
    std::vector<int32_t> relay_iters;   // [legs]
    int relay_bad_col = -1;             // as mem_bad_col, over all legs
    DeviceBuf relay_ag;                 // [legs][2][n]: a[] then gamma[] of every leg (mem_host.h: mem_form_a); rewritten by upload_relay
    DeviceBuf relay_it;                 // [legs] int32: relay_iters on the device
    DeviceBuf e_relay;                  // [legs][2][R * 64]: a and gamma of every slot, per leg (edge_relay_table_kernel, before every launch)
    DeviceBuf w_relay;                  // bp_wave_relay_kernel: [np + 2] the padded priors, then [legs][2][np] a and gamma of every column padded to np, per leg -- the relay's, or the memory's as one leg (before every launch)
    DeviceBuf relay_dec, relay_llr, relay_li, relay_cv, relay_state;  // the leg loop: a leg's outputs [batch][n] / [batch]; {best weight f64, solutions i32, iterations i32} per row
    // BP with guided decimation (ldpc_hip_bp_set_decimation): up to gd_max_rounds rounds of gd_round_iters min-sum iterations per
    // syndrome; a round that ends unsolved freezes the most reliable column at +-gd_freeze and keeps the messages.  gd_round_iters and gd_max_rounds
    // take max_iter's place.  decode_device looks at `variant` and sends the batch to decode_onchip_gd (host_onchip.h: the lane = edge kernels of
    // bp_edge_gd_kernel.h; with gd_lane_node also the lane = node kernel of bp_wave_gd_kernel.h; nothing else).  Decimation, relay and memory exclude one
    // another.  On the lane = edge kernels no device buffer of its own: the slot tables and e_prior are the plain decode's.
    int32_t gd_round_iters = 0, gd_max_rounds = 0;
    double gd_freeze = 0.0;
    bool gd_lane_node = false;  // ldpc_hip_bp_set_decimation_lane_node: codes beyond both lane = edge ladders go to bp_wave_gd_kernel (opt-in; a handle setting like small_mode, read only while the decimation is on)
    DeviceBuf w_gd;             // bp_wave_gd_kernel: [np + 2] the padded priors (before every launch; released when the decimation or the lane = node route is switched off)
    mutable int gd_route_known = -1, gd_route_method = 0, gd_route_mode = 0;  // gd_route's answer for this code under (bp_method, small_mode, gd_lane_node -- its setter forgets the answer), -1: not asked yet (the plans scan the matrix: once, not at every refusal check)
};

// h->counter: work_pool_bytes() of work counters for the on-chip BP kernels, then OSD_COUNTER_BYTES for BP + OSD -- {listed, next} of the first
// OSD pass at [0..1], of the second at [8..9] -- so that one fill clears both.  Everybody sizes the buffer with counter_bytes().
constexpr size_t OSD_COUNTER_BYTES = 64;
static_assert(OSD_COUNTER_BYTES >= 10 * sizeof(unsigned), "two pairs of OSD counters, the second at [8..9]");
static size_t counter_bytes() { return work_pool_bytes() + OSD_COUNTER_BYTES; }
static unsigned *osd_counter_ptr(const ldpc_hip_bp *h) { return (unsigned *)((char *)h->counter.p + work_pool_bytes()); }

// (bp_method, math_mode) of the handle as the compile-time pair <METHOD, MATH> the kernels are instantiated for -- min-sum has one
// arithmetic, product-sum two -- handed to `f` as two std::integral_constant<int, ...>:
//     kern = with_method_math(h, [&](auto M, auto F) { return pick_serial<M, F>(rows, cols); });
template <class Fn>
static auto with_method_math(const ldpc_hip_bp *h, Fn &&f) {
    if (h->bp_method == LDPC_HIP_MINIMUM_SUM) return f(std::integral_constant<int, LDPC_HIP_MINIMUM_SUM>{}, std::integral_constant<int, 0>{});
    if (h->math_mode == LDPC_HIP_MATH_FAST) return f(std::integral_constant<int, LDPC_HIP_PRODUCT_SUM>{}, std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, LDPC_HIP_PRODUCT_SUM>{}, std::integral_constant<int, 0>{});
}

// Memory min-sum: a[] and gamma[] of the priors and strengths the handle holds now -> mem_ag (the stream is idle: ldpc_hip_bp_set_memory and
// ldpc_hip_bp_set_channel wait for it first).  mem_bad_col: what a decode has to refuse (decode_gate).
static int upload_memory(ldpc_hip_bp *h) {
    const size_t n = (size_t)h->n;
    std::vector<double> ag(2 * (n ? n : 1), 0.0);
    h->mem_bad_col = mem_form_a(h->channel_probs.data(), h->mem_gamma.data(), h->n, ag.data());
    std::copy(h->mem_gamma.begin(), h->mem_gamma.end(), ag.begin() + (std::ptrdiff_t)n);
    int rc;
    if ((rc = h->mem_ag.ensure(sizeof(double) * ag.size()))) return rc;
    HIPCHK(hipMemcpy(h->mem_ag.p, ag.data(), sizeof(double) * ag.size(), hipMemcpyHostToDevice));
    return LDPC_HIP_OK;
}

// Relay-BP: a[] and gamma[] of every leg, and the legs' iteration limits -> relay_ag, relay_it (the stream is idle, as for upload_memory).
static int upload_relay(ldpc_hip_bp *h) {
    const size_t n = (size_t)h->n, legs = (size_t)h->relay_legs, n1 = n ? n : 1;
    std::vector<double> ag(legs * 2 * n1, 0.0);
    h->relay_bad_col = -1;
    for (size_t l = 0; l < legs; ++l) {
        const double *g = h->relay_gamma.data() + l * n;
        const int bad = mem_form_a(h->channel_probs.data(), g, h->n, ag.data() + l * 2 * n);
        if (bad >= 0 && (h->relay_bad_col < 0 || bad < h->relay_bad_col)) h->relay_bad_col = bad;
        std::copy(g, g + n, ag.begin() + (std::ptrdiff_t)(l * 2 * n + n));
    }
    int rc;
    if ((rc = h->relay_ag.ensure(sizeof(double) * ag.size())) || (rc = h->relay_it.ensure(sizeof(int32_t) * legs))) return rc;
    HIPCHK(hipMemcpy(h->relay_ag.p, ag.data(), sizeof(double) * ag.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->relay_it.p, h->relay_iters.data(), sizeof(int32_t) * legs, hipMemcpyHostToDevice));
    return LDPC_HIP_OK;
}

// tu_onchip.hip (host_onchip.h): which kernel decodes this handle's code with guided decimation -- 0 none, 1 bp_edge, 2 bp_edge8, and with
// gd_lane_node 3 / 4 bp_wave_gd with one wavefront / a team per syndrome.
// It looks at the matrix, the BP method, the small-code kernel mode and gd_lane_node only, and launches nothing.
int gd_route(const ldpc_hip_bp *h, int64_t batch);
// tu_onchip.hip (host_onchip.h): which kernels a row-prior decode of `batch` syndromes takes on the handle as it is set now -- plan_row_prior_route's
// answer, the one decode_onchip acts on: 0 per-pass, 1 bp_edge, 2 bp_edge8, 3 / 4 bp_wave_rp with one wavefront / a team per syndrome, 5 the slot kernel
int row_prior_route(const ldpc_hip_bp *h, int64_t batch, bool want_llr);

// THE gate of every decode entry point, before anything is staged or launched: what the handle is set up for that its modes -- float32 messages,
// and whichever of memory min-sum, Relay-BP and guided decimation is on -- cannot do (the rules and their texts: mode_host.h).  `what`: the call's own
// addition (row priors, soft syndromes, several GPUs) or nullptr; with_osd: the call runs the handle's osd_method / osd_order.  The on-chip
// kernels of gd_route are guided decimation's only routes: a code none of them takes is refused here, not decoded some other way.
static int decode_gate(const ldpc_hip_bp *h, const char *what, bool with_osd) {
    const Variant v = h->variant;
    const ModeState s = {h->bp_method, h->schedule == 1 && !h->random_serial, h->msg_dtype, v,
                         v == Variant::Memory ? h->mem_bad_col : v == Variant::Relay ? h->relay_bad_col : -1,
                         v != Variant::Decimation || gd_route(h, 0) != 0, h->small_mode, h->osd_method, h->osd_order, h->gd_lane_node};
    char msg[512];
    const int refused = mode_refusal(s, DecodeCall{what, with_osd}, msg, sizeof msg);
    return refused ? fail(refused, "%s", msg) : LDPC_HIP_OK;
}

static int upload_priors(ldpc_hip_bp *h) {
    ++h->priors_version;
    if (h->variant == Variant::Memory) { const int rc = upload_memory(h); if (rc) return rc; }  // a[] follows the priors
    if (h->variant == Variant::Relay) { const int rc = upload_relay(h); if (rc) return rc; }  // ... of every leg
    // bp.hpp:150-151, evaluated by the host libm so that priors are bit-identical to the reference's
    std::vector<double> llr0((size_t)h->n);
    for (int j = 0; j < h->n; ++j)
        llr0[(size_t)j] = std::log((1 - h->channel_probs[(size_t)j]) / h->channel_probs[(size_t)j]);
    HIPCHK(hipMemcpy(h->d_llr0, llr0.data(), sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice));
    for (int j = 0; j < h->n; ++j) llr0[(size_t)j] = std::log(1 / h->channel_probs[(size_t)j]);  // osd.hpp:134
    HIPCHK(hipMemcpy(h->d_osd_wt, llr0.data(), sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice));
    return 0;
}

// grid of the one-dimensional element-wise kernels (io_kernels.h): they run grid-stride loops, so the grid is capped --
// item counts like batch * n exceed what one launch dimension can carry for large batches of large codes
static dim3 flat_grid(size_t items) {
    size_t blocks = (items + 255) / 256;
    if (blocks > (1u << 22)) blocks = 1u << 22;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks);
}

// end of a call that only queued work: remembered so that a later change of stream is ordered after it (set_stream)
static int mark_queued(ldpc_hip_bp *h, int rc) {
    if (rc) return rc;
    HIPCHK(hipEventRecord(h->ev_done, h->stream));
    h->work_queued = true;
    return LDPC_HIP_OK;
}

static bool is_pinned_host_ptr(const void *p) {  // page-locked host memory (hipHostMalloc / hipHostRegister): a copy engine can write it directly
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

static bool is_device_ptr(const void *p) {
    if (!p) return true;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory reports an error: clear it
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// ---- what the chunked decodes of every schedule share (host_serial.h, host_stream.h) ------------------------------------------------------
// a kernel that wants more dynamic LDS than the 48 KiB it gets without asking
template <class Kernel>
static int set_dynamic_lds(Kernel kern, size_t bytes) {
    if (bytes > 48u * 1024u) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return LDPC_HIP_OK;
}

// tiles of per_tile bytes that fit into `margin` of the device memory that is free or held already by the buffers they will live in
static int tiles_that_fit(size_t per_tile, size_t held, double margin, int64_t *fit) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    *fit = (int64_t)((size_t)((double)(free_b + held) * margin) / (per_tile ? per_tile : 1));
    return LDPC_HIP_OK;
}

// tiles per chunk of a decode that takes its batch in pieces: all of them, up to what the caller allows (ldpc_hip_bp_set_tuning), one launch
// carries (`cap`) and memory holds.  `unit`: what a tile holds 64 of, for the message
static int chunk_tiles_that_fit(const ldpc_hip_bp *h, int64_t tiles_total, size_t per_tile, size_t held, double margin, int64_t cap, const char *unit, int64_t *chunk) {
    int64_t fit = 0;
    int rc;
    if ((rc = tiles_that_fit(per_tile, held, margin, &fit))) return rc;
    if (fit < 1) return fail(LDPC_HIP_ERR_NOMEM, "not enough device memory for one 64-%s tile", unit);
    *chunk = tiles_total;
    if (h->max_chunk_tiles > 0 && *chunk > h->max_chunk_tiles) *chunk = h->max_chunk_tiles;
    if (*chunk > cap) *chunk = cap;
    if (*chunk > fit) *chunk = fit;
    return LDPC_HIP_OK;
}

struct ChunkRange { int64_t tiles, b0, nb; };  // a chunk's tiles, its first row and its rows
static ChunkRange chunk_range(int64_t t0, int64_t chunk, int64_t tiles_total, int64_t batch) {
    ChunkRange c = {(tiles_total - t0 < chunk) ? tiles_total - t0 : chunk, t0 * LDPC_WAVE, 0};
    c.nb = (batch - c.b0 < c.tiles * LDPC_WAVE) ? batch - c.b0 : c.tiles * LDPC_WAVE;
    return c;
}

// the kernel time of a decode (ldpc_hip_bp_last_kernel_ms) starts over; prev_too: also what a two-pass decode before it left (evp0 / evp1)
static void reset_timing(ldpc_hip_bp *h, bool prev_too) {
    h->accumulated_ms = h->accumulated_persistent_ms = 0.f;
    h->timed = h->timed_mid = false;
    if (prev_too) h->timed_prev = h->timed_prev_mid = false;
}

// around a chunk's decode kernels: the chunk before it gives its time to accumulated_ms / accumulated_persistent_ms (its events are used again)
static int chunk_timing_begin(ldpc_hip_bp *h) {
    if (h->timed) {
        float prev = 0.f;
        HIPCHK(hipEventSynchronize(h->ev1));
        HIPCHK(hipEventElapsedTime(&prev, h->ev0, h->ev1));
        h->accumulated_ms += prev;
        if (h->timed_mid) {  // (the streamed decode: its persistent kernel's share, ev0 .. ev_mid)
            HIPCHK(hipEventElapsedTime(&prev, h->ev0, h->ev_mid));
            h->accumulated_persistent_ms += prev;
        }
    }
    h->timed_mid = false;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return LDPC_HIP_OK;
}
static int chunk_timing_end(ldpc_hip_bp *h) {
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// ---- what the two-pass decodes share (host_stream.h: decode_stream_repacked; host_f32.h: decode_f32_repacked) -----------------------------
// The pricing is described at decode_stream_repacked.  The handle has ONE histogram: one left by an FP64 decode may steer a float32 decode
// and the other way round (same code, same noise: same iteration counts up to the rows where the two arithmetics part); results do not
// depend on it, only where a decode is cut.
// *late_rows: rows (of the histogram's batch) still running 8 iterations into the second pass -- the stragglers its late rounds are for (-1: unknown)
static int stream_first_pass_length(ldpc_hip_bp *h, double *live_after, int64_t *late_rows, double gather_cost = 0.25) {
    *live_after = 0.5;
    *late_rows = -1;
    if (h->repack_iters > 0) return h->repack_iters < h->max_iter ? h->repack_iters : 0;
    // The previous decode's histogram, IF its copy has landed -- a look, never a wait (the *_async entry points must not block): a
    // caller that queues decodes back to back is steered by the last histogram that did land
    if (h->hist_pending) {
        const hipError_t q = hipEventQuery(h->ev_hist);
        if (q == hipSuccess) {
            std::memcpy(h->hist_landed, h->h_hist, sizeof h->hist_landed);
            h->hist_landed_max_iter = h->hist_max_iter;
            h->hist_landed_valid = true;
            h->hist_pending = false;
        } else {
            (void)hipGetLastError();  // hipErrorNotReady is not an error
        }
    }
    if (!h->hist_landed_valid || h->hist_landed_max_iter != h->max_iter) return 0;
    const int full = h->max_iter, top = full < 255 ? full : 255;
    double total = 0;
    for (int j = 0; j < 256; ++j) total += h->hist_landed[j];
    if (total <= 0) return 0;
    std::vector<double> F((size_t)top + 1, 0.0);  // F[j]: converged within j iterations
    double acc = 0;
    for (int j = 1; j <= top; ++j) { acc += h->hist_landed[j]; F[(size_t)j] = acc / total; }
    auto Fj = [&](int j) { return F[(size_t)(j < top ? j : top)]; };
    auto tile_runs = [&](int j) { return 1.0 - std::pow(Fj(j - 1), 64.0); };  // still going at iteration j
    double plain = 0;
    for (int j = 1; j <= full; ++j) plain += tile_runs(j);
    double best = plain, prefix = 0;
    int best_k = 0;
    for (int k = 1; k < full && k <= top; ++k) {
        prefix += tile_runs(k);
        const double live = 1.0 - Fj(k);
        if (k < 2 || live <= 0.0 || live > 0.6) continue;
        double rest = 0;
        for (int j = k + 1; j <= full; ++j) {
            const double g = (Fj(j - 1) - Fj(k)) / live;  // of the rows alive after k: done within j - 1
            const double r = 1.0 - std::pow(g < 0 ? 0 : g, 64.0);
            rest += r;
            if (r < 1e-9 && j > top) break;
        }
        const double cost = prefix + gather_cost * (1.0 + live) + 0.1 + live * rest;
        if (cost < best) { best = cost; best_k = k; *live_after = live; }
    }
    if (best_k > 0) {
        double late = h->hist_landed[0];
        for (int j = best_k + 9; j < 256; ++j) late += h->hist_landed[j];
        *late_rows = (int64_t)late;
    }
    return best < 0.97 * plain ? best_k : 0;
}

static int stream_leave_histogram(ldpc_hip_bp *h, const int32_t *iters, const uint8_t *conv, int64_t batch) {
    int rc;
    if ((rc = h->sp_hist.ensure(256 * sizeof(unsigned)))) return rc;
    if (!h->h_hist) HIPCHK(hipHostMalloc((void **)&h->h_hist, 256 * sizeof(unsigned), hipHostMallocDefault));
    HIPCHK(hipMemsetAsync(h->sp_hist.p, 0, 256 * sizeof(unsigned), h->stream));
    int64_t blocks = (batch + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    LDPC_LAUNCH(iteration_histogram_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, iters, conv, batch, (unsigned *)h->sp_hist.p);
    HIPCHK(hipMemcpyAsync(h->h_hist, h->sp_hist.p, 256 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipEventRecord(h->ev_hist, h->stream));
    h->hist_pending = true;
    h->hist_max_iter = h->max_iter;
    return LDPC_HIP_OK;
}

// rows_dev[0] = rows listed by osd_collect_kernel, rows_dev[1] = their 64-row tiles (BpArgs::rows_dev)
LDPC_IO_KERNEL void repack_rows_kernel(const unsigned *__restrict__ counters, unsigned *__restrict__ rows_dev) {
    const unsigned c = counters[0];
    rows_dev[0] = c;
    rows_dev[1] = (c + LDPC_WAVE - 1) / LDPC_WAVE;
}


// ---- what the translation units call in each other (device pointers, on h->stream) -------------------------------------------------
// tu_stream.hip: the dispatch of a batch to a kernel family, and the streamed kernels themselves
int decode_device(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv);
// tu_onchip.hip: ONE syndrome in the handle's host-mapped block (already copied in) through the resident workgroup; *took = false: not
// applicable (then the ordinary path).  resident_retire: the resident workgroup leaves now (destroy, or a change it must not outlive)
int decode_onchip_resident(ldpc_hip_bp *h, bool want_llr, bool *took);
void resident_retire(ldpc_hip_bp *h);
// tu_onchip.hip: the kernels that keep a syndrome's messages on chip; *took = false: no such kernel applies to this matrix
int decode_onchip(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took);
// tu_onchip.hip: Relay-BP on chip, all legs in one launch -- the lane = edge relay kernels (bp_edge_relay_kernel.h, tu_onchip_relay.hip) for the codes
// plan_edge / plan_edge8 take, the lane = node kernel (bp_wave_relay_kernel.h, tu_onchip_wave_relay.hip) for those plan_wave_relay takes, by the small-code
// kernel mode (plan_relay_route); *took = false: decode_relay (host_stream.h) runs its leg loop
int decode_onchip_relay(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took);
// tu_onchip.hip: BP with guided decimation, all rounds in one launch -- the lane = edge decimation kernels (bp_edge_gd_kernel.h, tu_onchip_gd.hip) for the
// codes plan_edge / plan_edge8 take, with gd_lane_node the lane = node kernel (bp_wave_gd_kernel.h, tu_onchip_wave_gd.hip) for those plan_wave_gd takes
// (gd_route); any other code: LDPC_HIP_ERR_UNSUPPORTED, nothing launched
int decode_onchip_gd(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv);
// tu_serial.hip: serial / serial_relative / random serial schedules, soft-syndrome decoding
int decode_serial(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv);
int soft_info_device(ldpc_hip_bp *h, const double *soft, int64_t batch, double cutoff, double sigma, uint8_t *decoding, double *llr,
                     int32_t *iters, uint8_t *conv, double *soft_out);
// tu_f32.hip: the float32 message mode (min-sum, parallel schedule)
int decode_f32(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv);
// tu_onchip.hip: the float32 mode's on-chip routes (plan_f32_route) -- bp_edge_f32_kernel, bp_edge8_f32_kernel (instantiated in tu_onchip_f32.hip) for the
// codes plan_edge / plan_edge8 take, with f32_lane_node bp_wave_f32_kernel (tu_onchip_wave_f32.hip) for those plan_wave_f32 takes; *took = false: none
// does (decode_f32 then runs its per-pass kernels)
int decode_onchip_f32(ldpc_hip_bp *h, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr, int32_t *iters, uint8_t *conv, bool *took);
// bp_hip.hip (host_decode_abi.h): the body of ldpc_hip_bp_decode_b8 on device pointers -- unpack, decode, zero-shot shortcut, observables / packed
// decodings -- queued on h->stream without waiting (ldpc_hip_bp_simulate_b8 runs it per chunk)
int decode_b8_device(ldpc_hip_bp *h, const uint8_t *d_dets_b8, int64_t batch, int32_t with_osd, uint8_t *d_obs_b8, uint8_t *d_decoding_b8,
                     int32_t *d_iters, uint8_t *d_conv);
// tu_dem.hip: the column view of the observables matrix for dem_sample_b8_kernel, from the handle's host copy (ldpc_hip_bp_set_observables calls it
// when a sampler is set already, ldpc_hip_bp_set_sampler when observables are)
int dem_upload_obs_csc(ldpc_hip_bp *h);
// tu_osd.hip: BP followed by ordered-statistics post-processing of the rows it left unconverged
int bposd_device(ldpc_hip_bp *h, int osd_method, int osd_order, const uint8_t *synd, int64_t batch, uint8_t *decoding, double *llr,
                 int32_t *iters, uint8_t *conv);
