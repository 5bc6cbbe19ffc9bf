// A caller that includes Reduce.h only: the total and the largest |v| of a small matrix with an empty row, in both
// precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_reduce.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Reduce.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -2 0; 0 0 0; 5 0 -7]
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2};
    const T v[4] = {1, -2, 5, -7};
    speck_dcsr da{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> A;
    A.adopt(da);
    speck_reduce_info info{};
    double total = 99.0;
    spECK::Reduce(A, SPECK_REDUCE_SUM, nullptr, &total, config, &info);
    if (total != -3.0 || info.rows_empty != 1 || info.rows_split != 0 || info.tiles != 1 || info.entries != 4) return 2;
    spECK::Reduce(A, SPECK_REDUCE_ABS_MAX, nullptr, &total, config);
    if (total != 7.0) return 3;
    spECK::Reduce(A, SPECK_REDUCE_MIN, nullptr, &total, config);
    if (total != -7.0) return 4;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "reduce caller ok\n" : "reduce caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("reduce caller: %s\n", e.what());
        return 100;
    }
}
