// host_dem.h -- C ABI: sampling a detector error model on the device, counting mismatching rows, and the sample -> decode -> compare loop
// (include/ldpc_hip.h: ldpc_hip_bp_set_sampler, ldpc_hip_bp_sample_b8, ldpc_hip_count_mismatch_b8, ldpc_hip_bp_simulate_b8)
// Part of libldpc_hip.so: included by tu_dem.hip (one translation unit).  Kernels: dem_sample_kernels.h; host arithmetic: dem_host.h.
#pragma once

#include "dem_host.h"

int dem_upload_obs_csc(ldpc_hip_bp *h) {
    std::vector<int32_t> col_ptr, csc_row;
    if (!dem_csr_to_csc(h->obs_k, h->n, h->h_obs_row_ptr.data(), h->h_obs_col_idx.data(), &col_ptr, &csc_row))
        return fail(LDPC_HIP_ERR_INVALID, "observables matrix: bad row pointers or column indices");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    int rc;
    if ((rc = h->dem_obs_col_ptr.ensure(sizeof(int32_t) * col_ptr.size()))) return rc;
    if ((rc = h->dem_obs_csc_row.ensure(sizeof(int32_t) * (csc_row.size() ? csc_row.size() : 1)))) return rc;
    HIPCHK(hipMemcpy(h->dem_obs_col_ptr.p, col_ptr.data(), sizeof(int32_t) * col_ptr.size(), hipMemcpyHostToDevice));
    if (!csc_row.empty()) HIPCHK(hipMemcpy(h->dem_obs_csc_row.p, csc_row.data(), sizeof(int32_t) * csc_row.size(), hipMemcpyHostToDevice));
    return LDPC_HIP_OK;
}

// strips of one wavefront in 32-bit words; refused (nothing launched) when they pass what 64 KiB a workgroup give it
static int dem_lds_words(const ldpc_hip_bp *h, bool with_obs, int *words) {
    const int64_t w = ((int64_t)h->m + 31) / 32 + (with_obs ? ((int64_t)h->obs_k + 31) / 32 : 0);
    if (w > DEM_LDS_WORDS_PER_WAVE)
        return fail(LDPC_HIP_ERR_UNSUPPORTED,
                    "dem_sample_b8_kernel keeps a shot's detectors and observables in LDS: ceil(m / 32) + ceil(k / 32) = %lld words, at most %d "
                    "(m + k <= %d bits; 64 KiB a workgroup of %d wavefronts); there is no global-memory fallback",
                    (long long)w, DEM_LDS_WORDS_PER_WAVE, DEM_LDS_WORDS_PER_WAVE * 32, DEM_WAVES);
    *words = (int)w;
    return LDPC_HIP_OK;
}

// device pointers, queued on h->stream; the caller has checked sampler / observables / batch > 0
static int dem_sample_device(ldpc_hip_bp *h, uint64_t seed, int64_t shot0, int64_t batch, uint8_t *d_dets, uint8_t *d_obs, uint8_t *d_errs) {
    int words = 0, rc;
    if ((rc = dem_lds_words(h, d_obs != nullptr, &words))) return rc;
    DemSampleArgs a;
    a.col_ptr = h->d_col_ptr; a.csc_row = h->d_csc_row;
    a.obs_col_ptr = (const int32_t *)h->dem_obs_col_ptr.p; a.obs_csc_row = (const int32_t *)h->dem_obs_csc_row.p;
    a.thr = (const uint64_t *)h->dem_thr.p;
    a.m = h->m; a.n = h->n; a.k = d_obs ? h->obs_k : 0;
    a.seed = seed; a.shot0 = shot0; a.batch = batch;
    a.dets = d_dets; a.obs = d_obs && h->obs_k > 0 ? d_obs : nullptr; a.errs = d_errs;
    // a wavefront per shot while they are few; beyond 8 workgroups a compute unit the wavefronts loop (switch DEM_GRID k > 0: at most k
    // workgroups -- the tests reach the loop at 3000 shots with it)
    int64_t grid = (batch + DEM_WAVES - 1) / DEM_WAVES;
    const int64_t cap = h->sw("DEM_GRID") > 0 ? h->sw("DEM_GRID") : 256 * 8;
    if (grid > cap) grid = cap;
    if (!a.obs) words = (h->m + 31) / 32;
    const size_t lds = ((size_t)DEM_WAVES * (size_t)words * 4 + 15) & ~(size_t)15;
    if ((rc = set_dynamic_lds(dem_sample_b8_kernel, lds))) return rc;
    LDPC_LAUNCH(dem_sample_b8_kernel, dim3((unsigned)grid), dim3(DEM_WAVES * 64), lds, h->stream, a);
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

// device pointers, queued on h->stream: *d_count += rows that differ (y == nullptr: rows of x that are zero when `invert`, else nonzero)
static int dem_count_device(ldpc_hip_bp *h, const uint8_t *x, const uint8_t *y, int64_t batch, int bits, int invert, unsigned long long *d_count,
                            uint8_t *d_flags) {
    int64_t blocks = (batch + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    LDPC_LAUNCH(mismatch_b8_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, x, y, batch, bits, invert, d_count, d_flags);
    HIPCHK(hipGetLastError());
    return LDPC_HIP_OK;
}

extern "C" {

int ldpc_hip_bp_set_sampler(ldpc_hip_bp *h, const double *probs) {
    if (!h) return fail(LDPC_HIP_ERR_INVALID, "null handle");
    const double *p = probs ? probs : h->channel_probs.data();
    std::vector<uint64_t> thr((size_t)(h->n ? h->n : 1));
    const int64_t bad = dem_thresholds(p, h->n, thr.data());
    if (bad >= 0) return fail(LDPC_HIP_ERR_INVALID, "sampler: probability %lld is outside [0, 1] or NaN", (long long)bad);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    int rc;
    if ((rc = h->dem_thr.ensure(sizeof(uint64_t) * thr.size()))) return rc;
    if (h->n) HIPCHK(hipMemcpy(h->dem_thr.p, thr.data(), sizeof(uint64_t) * (size_t)h->n, hipMemcpyHostToDevice));
    h->sampler_set = true;
    if (h->obs_k >= 0) return dem_upload_obs_csc(h);  // (the observables came first: their column view is built here)
    return LDPC_HIP_OK;
}

int ldpc_hip_bp_sample_b8(ldpc_hip_bp *h, uint64_t seed, int64_t shot0, int64_t batch, uint8_t *dets_b8, uint8_t *obs_b8, uint8_t *errors_b8) {
    if (!h) return fail(LDPC_HIP_ERR_INVALID, "null handle");
    if (batch < 0 || shot0 < 0) return fail(LDPC_HIP_ERR_INVALID, "negative batch or shot0");
    if (!h->sampler_set) return fail(LDPC_HIP_ERR_INVALID, "ldpc_hip_bp_set_sampler was never called");
    if (obs_b8 && h->obs_k < 0) return fail(LDPC_HIP_ERR_INVALID, "obs_b8 requested but ldpc_hip_bp_set_observables was never called");
    if (batch == 0) return LDPC_HIP_OK;
    if (!dets_b8 && h->m > 0) return fail(LDPC_HIP_ERR_INVALID, "null detection-event buffer");
    int words = 0, rc;
    if ((rc = dem_lds_words(h, obs_b8 != nullptr, &words))) return rc;  // (before anything is staged)
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)batch, mb = ((size_t)h->m + 7) / 8, nb = ((size_t)h->n + 7) / 8, kb = obs_b8 ? ((size_t)h->obs_k + 7) / 8 : 0;
    uint8_t *d_d = dets_b8, *d_o = obs_b8, *d_e = errors_b8;
    const bool h_d = dets_b8 && !is_device_ptr(dets_b8), h_o = obs_b8 && !is_device_ptr(obs_b8), h_e = errors_b8 && !is_device_ptr(errors_b8);
    if (h_d) { if ((rc = h->sim_dets.ensure(B * mb ? B * mb : 1))) return rc; d_d = (uint8_t *)h->sim_dets.p; }
    if (h_o) { if ((rc = h->sim_obs.ensure(B * kb ? B * kb : 1))) return rc; d_o = (uint8_t *)h->sim_obs.p; }
    if (h_e) { if ((rc = h->sim_err.ensure(B * nb ? B * nb : 1))) return rc; d_e = (uint8_t *)h->sim_err.p; }
    if ((rc = dem_sample_device(h, seed, shot0, batch, d_d, d_o, d_e))) return rc;
    if (h_d && mb) HIPCHK(hipMemcpyAsync(dets_b8, d_d, B * mb, hipMemcpyDeviceToHost, h->stream));
    if (h_o && kb) HIPCHK(hipMemcpyAsync(obs_b8, d_o, B * kb, hipMemcpyDeviceToHost, h->stream));
    if (h_e && nb) HIPCHK(hipMemcpyAsync(errors_b8, d_e, B * nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LDPC_HIP_OK;
}

int ldpc_hip_count_mismatch_b8(ldpc_hip_bp *h, const uint8_t *a_b8, const uint8_t *b_b8, int64_t batch, int32_t bits, uint64_t *count,
                               uint8_t *row_flags) {
    if (!h) return fail(LDPC_HIP_ERR_INVALID, "null handle");
    if (batch < 0 || bits < 0) return fail(LDPC_HIP_ERR_INVALID, "negative batch or bits");
    if (!count) return fail(LDPC_HIP_ERR_INVALID, "null count");
    HIPCHK(hipSetDevice(h->device));
    const size_t B = (size_t)batch, nb = ((size_t)bits + 7) / 8;
    if (batch == 0 || bits == 0) {  // nothing can differ
        if (is_device_ptr(count)) HIPCHK(hipMemsetAsync(count, 0, sizeof(uint64_t), h->stream));
        else *count = 0;
        if (row_flags && batch) {
            if (is_device_ptr(row_flags)) HIPCHK(hipMemsetAsync(row_flags, 0, B, h->stream));
            else std::memset(row_flags, 0, B);
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        return LDPC_HIP_OK;
    }
    if (!a_b8 || !b_b8) return fail(LDPC_HIP_ERR_INVALID, "null buffer");
    int rc;
    // Host operands are staged in the buffers ldpc_hip_bp_simulate_b8 uses per chunk (sim_obs, sim_pred, sim_conv, sim_count).  That is safe
    // because both entry points wait for the stream before they return and a handle serves one call at a time; an asynchronous form of
    // either would need staging of its own.
    const bool h_a = !is_device_ptr(a_b8), h_b = !is_device_ptr(b_b8), h_c = !is_device_ptr(count), h_f = row_flags && !is_device_ptr(row_flags);
    const uint8_t *d_a = a_b8, *d_b = b_b8;
    uint8_t *d_f = row_flags;
    if (h_a) {
        if ((rc = h->sim_obs.ensure(B * nb))) return rc;
        HIPCHK(hipMemcpyAsync(h->sim_obs.p, a_b8, B * nb, hipMemcpyHostToDevice, h->stream));
        d_a = (const uint8_t *)h->sim_obs.p;
    }
    if (h_b) {
        if ((rc = h->sim_pred.ensure(B * nb))) return rc;
        HIPCHK(hipMemcpyAsync(h->sim_pred.p, b_b8, B * nb, hipMemcpyHostToDevice, h->stream));
        d_b = (const uint8_t *)h->sim_pred.p;
    }
    if (h_f) { if ((rc = h->sim_conv.ensure(B))) return rc; d_f = (uint8_t *)h->sim_conv.p; }
    if ((rc = h->sim_count.ensure(2 * sizeof(uint64_t)))) return rc;
    unsigned long long *d_c = h_c ? (unsigned long long *)h->sim_count.p : (unsigned long long *)count;
    HIPCHK(hipMemsetAsync(d_c, 0, sizeof(uint64_t), h->stream));
    if ((rc = dem_count_device(h, d_a, d_b, batch, bits, 0, d_c, d_f))) return rc;
    if (h_c) HIPCHK(hipMemcpyAsync(count, d_c, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (h_f) HIPCHK(hipMemcpyAsync(row_flags, d_f, B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return LDPC_HIP_OK;
}

int ldpc_hip_bp_simulate_b8(ldpc_hip_bp *h, uint64_t seed, int64_t shot0, int64_t shots, int64_t chunk, int32_t with_osd, uint64_t *out) {
    if (!h) return fail(LDPC_HIP_ERR_INVALID, "null handle");
    if (shots < 0 || shot0 < 0) return fail(LDPC_HIP_ERR_INVALID, "negative shots or shot0");
    if (!out) return fail(LDPC_HIP_ERR_INVALID, "null output");
    if (!h->sampler_set) return fail(LDPC_HIP_ERR_INVALID, "ldpc_hip_bp_set_sampler was never called");
    if (h->obs_k < 0) return fail(LDPC_HIP_ERR_INVALID, "ldpc_hip_bp_set_observables was never called");
    { const int refused = decode_gate(h, nullptr, with_osd != 0); if (refused) return refused; }
    out[0] = out[1] = 0;
    if (shots == 0) return LDPC_HIP_OK;
    int words = 0, rc;
    if ((rc = dem_lds_words(h, true, &words))) return rc;
    if (chunk <= 0) chunk = 65536;
    if (chunk > shots) chunk = shots;
    HIPCHK(hipSetDevice(h->device));
    const size_t C = (size_t)chunk, mb = ((size_t)h->m + 7) / 8, kb = ((size_t)h->obs_k + 7) / 8;
    if ((rc = h->sim_dets.ensure(C * mb ? C * mb : 1))) return rc;
    if ((rc = h->sim_obs.ensure(C * kb ? C * kb : 1))) return rc;
    if ((rc = h->sim_pred.ensure(C * kb ? C * kb : 1))) return rc;
    if ((rc = h->sim_conv.ensure(C))) return rc;
    if ((rc = h->sim_count.ensure(2 * sizeof(uint64_t)))) return rc;
    uint8_t *d_dets = (uint8_t *)h->sim_dets.p, *d_obs = (uint8_t *)h->sim_obs.p, *d_pred = (uint8_t *)h->sim_pred.p, *d_conv = (uint8_t *)h->sim_conv.p;
    unsigned long long *d_count = (unsigned long long *)h->sim_count.p;
    HIPCHK(hipMemsetAsync(d_count, 0, 2 * sizeof(uint64_t), h->stream));
    for (int64_t done = 0; done < shots; done += chunk) {  // sample -> decode -> predict observables -> count, all on h->stream
        const int64_t nb = shots - done < chunk ? shots - done : chunk;
        if ((rc = dem_sample_device(h, seed, shot0 + done, nb, d_dets, d_obs, nullptr))) return rc;
        if ((rc = decode_b8_device(h, d_dets, nb, with_osd, d_pred, nullptr, nullptr, d_conv))) return rc;
        if (kb && (rc = dem_count_device(h, d_obs, d_pred, nb, h->obs_k, 0, d_count, nullptr))) return rc;
        if ((rc = dem_count_device(h, d_conv, nullptr, nb, 8, 1, d_count + 1, nullptr))) return rc;
    }
    uint64_t host[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(host, d_count, sizeof host, hipMemcpyDeviceToHost, h->stream));  // nothing but the two counters comes back
    HIPCHK(hipStreamSynchronize(h->stream));
    out[0] = host[0];
    out[1] = host[1];
    return LDPC_HIP_OK;
}

}  // extern "C"
