// Stand-alone check of ldpc_amd/csrc/dem_host.h -- the host arithmetic of the detector-error-model sampler -- meant to run under the
// host sanitizers (nothing of it touches a GPU or Python):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I ldpc_amd/csrc tools/dem_host_check.cpp -o dem_host_check
//     ./dem_host_check          (exit status 0 and "dem_host_check ok"; tests/test_dem_sampler_twin.py builds and runs it)
#include <cstdio>
#include <limits>

#include "dem_host.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    const uint64_t two53 = 1ull << 53;
    // the values tests/test_dem_sampler_twin.py pins for prng.bernoulli_thresholds
    const double p[] = {0.0, 1.0, 0.5, 1e-300, 1.0 - 1.0 / 9007199254740992.0, 0.001, 0.09, 1.0 / 9007199254740992.0, 0.5 / 9007199254740992.0};
    const int np_ = (int)(sizeof p / sizeof p[0]);
    std::vector<uint64_t> t((size_t)np_);
    EXPECT(dem_thresholds(p, np_, t.data()) == -1);
    EXPECT(t[0] == 0 && t[1] == two53 && t[2] == two53 / 2 && t[3] == 1 && t[4] == two53 - 1 && t[7] == 1 && t[8] == 1);
    EXPECT(t[5] == (uint64_t)std::ceil(0.001 * 9007199254740992.0) && t[6] == (uint64_t)std::ceil(0.09 * 9007199254740992.0));
    const double bad[] = {0.25, -1e-9, 0.5};
    EXPECT(dem_thresholds(bad, 3, t.data()) == 1);
    const double bad2[] = {0.25, 0.5, 1.0 + 1e-12};
    EXPECT(dem_thresholds(bad2, 3, t.data()) == 2);
    const double bad3[] = {std::numeric_limits<double>::quiet_NaN()};
    EXPECT(dem_thresholds(bad3, 1, t.data()) == 0);
    const double bad4[] = {std::numeric_limits<double>::infinity()};
    EXPECT(dem_thresholds(bad4, 1, t.data()) == 0);
    EXPECT(dem_thresholds(p, 0, nullptr) == -1);

    // rows -> columns: 3 x 5, an empty row, an empty column, unsorted indices and a repeated entry
    const int32_t row_ptr[] = {0, 4, 4, 7}, col_idx[] = {4, 0, 2, 2, 0, 1, 4};
    std::vector<int32_t> col_ptr, csc_row;
    EXPECT(dem_csr_to_csc(3, 5, row_ptr, col_idx, &col_ptr, &csc_row));
    const std::vector<int32_t> want_ptr = {0, 2, 3, 5, 5, 7}, want_row = {0, 2, 2, 0, 0, 0, 2};
    EXPECT(col_ptr == want_ptr);
    EXPECT(csc_row == want_row);
    // no rows at all (k = 0: the row pointer holds one entry), and no columns
    const int32_t one[] = {0};
    EXPECT(dem_csr_to_csc(0, 4, one, nullptr, &col_ptr, &csc_row) && col_ptr == std::vector<int32_t>(5, 0) && csc_row.empty());
    EXPECT(dem_csr_to_csc(0, 0, one, nullptr, &col_ptr, &csc_row) && col_ptr == std::vector<int32_t>(1, 0));
    // refused, without reading past anything: an index out of range, a negative one, row pointers that decrease or do not start at 0
    const int32_t rp2[] = {0, 2}, ci_hi[] = {1, 5}, ci_lo[] = {-1, 1};
    EXPECT(!dem_csr_to_csc(1, 5, rp2, ci_hi, &col_ptr, &csc_row));
    EXPECT(!dem_csr_to_csc(1, 5, rp2, ci_lo, &col_ptr, &csc_row));
    const int32_t rp3[] = {0, 2, 1}, ci3[] = {0, 1};
    EXPECT(!dem_csr_to_csc(2, 5, rp3, ci3, &col_ptr, &csc_row));
    const int32_t rp4[] = {1, 2};
    EXPECT(!dem_csr_to_csc(1, 5, rp4, ci3, &col_ptr, &csc_row));

    if (failures) return 1;
    std::printf("dem_host_check ok\n");
    return 0;
}
