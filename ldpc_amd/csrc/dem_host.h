// dem_host.h -- host arithmetic of the detector-error-model sampler: probabilities -> 53-bit thresholds, rows -> columns of a sparse matrix.
// Plain C++ with no HIP in it, so that a stand-alone program can include it and run under a host sanitizer (tools/dem_host_check.cpp);
// host_dem.h is the only other user.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

// T = min(max(ceil(p * 2^53), 0), 2^53): `(sm64 >> 11) < T` fires with probability p (twin of ldpc_amd/prng.py: bernoulli_threshold).  The product
// with a power of two and the ceil are exact in float64.  false: p is outside [0, 1] or NaN.
static inline bool dem_threshold(double p, uint64_t *t) {
    if (!(p >= 0.0 && p <= 1.0)) return false;
    const double two53 = 9007199254740992.0;
    double c = std::ceil(p * two53);
    if (c < 0.0) c = 0.0;
    if (c > two53) c = two53;
    *t = (uint64_t)c;
    return true;
}

// thresholds of p[0 .. n): -1 when all are probabilities, else the index of the first that is not (out[] is then valid below it only)
static inline int64_t dem_thresholds(const double *p, int64_t n, uint64_t *out) {
    for (int64_t j = 0; j < n; ++j)
        if (!dem_threshold(p[j], &out[j])) return j;
    return -1;
}

// Column view of a k x n matrix given by rows (CSR, column indices in [0, n), any order, repeats allowed): column j's rows at
// [col_ptr[j], col_ptr[j + 1]) of csc_row, ascending (a repeated entry is repeated).  false: an index outside [0, n) or row pointers that decrease.
static inline bool dem_csr_to_csc(int32_t k, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, std::vector<int32_t> *col_ptr,
                                  std::vector<int32_t> *csc_row) {
    col_ptr->assign((size_t)n + 1, 0);
    csc_row->clear();
    if (k < 0 || n < 0 || (k > 0 && row_ptr[0] != 0)) return false;
    for (int32_t i = 0; i < k; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return false;
        for (int32_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) return false;
            ++(*col_ptr)[(size_t)col_idx[e] + 1];
        }
    }
    for (int32_t j = 0; j < n; ++j) (*col_ptr)[(size_t)j + 1] += (*col_ptr)[(size_t)j];
    csc_row->resize((size_t)(*col_ptr)[(size_t)n]);
    std::vector<int32_t> fill(col_ptr->begin(), col_ptr->end() - 1);
    for (int32_t i = 0; i < k; ++i)
        for (int32_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) (*csc_row)[(size_t)fill[(size_t)col_idx[e]]++] = i;
    return true;
}
