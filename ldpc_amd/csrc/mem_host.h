// mem_host.h -- host arithmetic of memory min-sum BP (ldpc_hip_bp_set_memory): the strengths validated, a[] formed, the priors it needs finite
// Plain C++ with no HIP in it, so that a stand-alone program can include it and run under a host sanitizer (tools/mem_host_check.cpp);
// host_setup.h calls the same functions.
#pragma once

#include <cmath>
#include <cstdint>

// Memory strengths gamma[0 .. n): each finite and in [-1, 1).  -> -1 if all are, else the first index that is not.
inline int mem_gamma_first_invalid(const double *gamma, int n) {
    for (int j = 0; j < n; ++j)
        if (!(std::isfinite(gamma[j]) && gamma[j] >= -1.0 && gamma[j] < 1.0)) return j;
    return -1;
}

// a[j] = (1 - gamma[j]) * L0[j] with L0[j] = log((1 - p[j]) / p[j]) as upload_priors forms it: the subtraction rounded, then the product --
// two roundings, no FMA (the library is built with -ffp-contract=off; the operands are spelled out so that no other build contracts them).
// gamma[j] == 0: a[j] = L0[j] itself (1.0 * x is x, the infinities of p = 0 / 1 included) -- the kernels then take a[j] for the prior by a
// select, without arithmetic.  With 1 - gamma > 0 -- at least 2^-53 -- and |L0| >= 1.1e-16 where it is not zero, the product neither
// underflows nor changes sign: a[j] is never -0.0 (L0 = log(1.0) = +0.0 at p = 0.5 gives +0.0).
// -> -1, or the first column with gamma != 0 whose L0 is not finite (p of 0 or 1, or outside [0, 1]): a decode must refuse it.
inline int mem_form_a(const double *p, const double *gamma, int n, double *a) {
    int bad = -1;
    for (int j = 0; j < n; ++j) {
        const double l0 = std::log((1 - p[j]) / p[j]);
        if (gamma[j] == 0.0) { a[j] = l0; continue; }
        volatile double w = 1.0 - gamma[j];
        volatile double prod = w * l0;
        a[j] = prod;
        if (bad < 0 && !std::isfinite(l0)) bad = j;
    }
    return bad;
}
