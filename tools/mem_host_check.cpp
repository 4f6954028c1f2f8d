// Stand-alone check of ldpc_amd/csrc/mem_host.h -- the host arithmetic of memory min-sum BP (ldpc_hip_bp_set_memory: the strengths validated,
// a[] formed) -- meant to run under the host sanitizers (nothing of it touches a GPU or Python):
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I ldpc_amd/csrc tools/mem_host_check.cpp -o mem_host_check
//     ./mem_host_check [p gamma]...     (exit status 0 and "mem_host_check ok"; tests/test_mem_bp_restatement.py builds and runs it)
// Every (p, gamma) pair given -- C99 hexadecimal floating point, as float.hex() writes it -- is answered with a line "a <bits of a[j] in hex>";
// the line "bad <index>" says what mem_form_a returned.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "mem_host.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static uint64_t bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

int main(int argc, char **argv) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // validity: finite and in [-1, 1)
    const double ok[] = {-1.0, 0.0, -0.0, 0.35, 1.0 - 1.0 / 9007199254740992.0, -0.24};
    EXPECT(mem_gamma_first_invalid(ok, 6) == -1);
    EXPECT(mem_gamma_first_invalid(ok, 0) == -1);
    for (double bad : {1.0, -1.5, nan, inf, -inf, 1.0000000000000002}) {
        const double g[] = {0.5, bad, 0.0};
        EXPECT(mem_gamma_first_invalid(g, 3) == 1);
    }
    // a[]: gamma == 0 keeps the prior, infinities included; elsewhere (1 - gamma) * log((1 - p) / p); never -0.0
    const double p[] = {0.0, 1.0, 0.5, 1e-300, 0.03, 0.5, 0.2, 0.5};
    const double g[] = {0.0, 0.0, 0.35, 0.66, -0.24, -1.0, 0.0, 1.0 - 1.0 / 9007199254740992.0};
    double a[8];
    EXPECT(mem_form_a(p, g, 8, a) == -1);
    EXPECT(a[0] == inf && a[1] == -inf);
    EXPECT(bits(a[2]) == 0 && bits(a[5]) == 0 && bits(a[7]) == 0);  // +0.0, not -0.0
    EXPECT(a[3] == (1.0 - 0.66) * std::log((1 - 1e-300) / 1e-300));
    EXPECT(a[4] == (1.0 - -0.24) * std::log((1 - 0.03) / 0.03));
    EXPECT(a[6] == std::log((1 - 0.2) / 0.2));
    const double g_bad[] = {0.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    EXPECT(mem_form_a(p, g_bad, 8, a) == 1);  // nonzero strength on p = 1
    const double g_bad0[] = {-0.5, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    EXPECT(mem_form_a(p, g_bad0, 8, a) == 0);  // ... the FIRST such column
    EXPECT(mem_form_a(p, g, 0, nullptr) == -1);

    // the caller's pairs
    const int n = (argc - 1) / 2;
    if ((argc - 1) % 2) { std::printf("arguments come in (p, gamma) pairs\n"); return 2; }
    std::vector<double> pp((size_t)n), gg((size_t)n), aa((size_t)n);
    for (int j = 0; j < n; ++j) {
        pp[(size_t)j] = std::strtod(argv[1 + 2 * j], nullptr);
        gg[(size_t)j] = std::strtod(argv[2 + 2 * j], nullptr);
    }
    const int bad = mem_form_a(pp.data(), gg.data(), n, aa.data());
    for (int j = 0; j < n; ++j) std::printf("a %016" PRIx64 "\n", bits(aa[(size_t)j]));
    std::printf("bad %d\n", bad);

    if (failures) return 1;
    std::printf("mem_host_check ok\n");
    return 0;
}
