// A caller that includes SpMV.h only: y = A x and y = 2 A x - 3 y of a small matrix with an empty row, in both precisions.
// Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_spmv.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "SpMV.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -2 0; 0 0 0; 5 0 -7], x = (3, 4, 5); the vectors travel as the data arrays of two 1 x 3 matrices of doubles
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2}, vro[2] = {0, 3}, vci[3] = {0, 1, 2};
    const T v[4] = {1, -2, 5, -7};
    const double x[3] = {3, 4, 5}, y0[3] = {1, 1, 1};
    speck_dcsr da{}, dx{}, dy{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dx, 1, 3, 3, vro, vci, x, 8) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dy, 1, 3, 3, vro, vci, y0, 8) != SPECK_OK) return 1;
    dCSR<T> A;
    A.adopt(da);
    speck_spmv_info info{};
    double y[3];
    spECK::SpMV(A, static_cast<const double*>(dx.data), static_cast<double*>(dy.data), config, 1.0, 0.0, &info);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 8) != SPECK_OK) return 1;
    if (y[0] != -5.0 || y[1] != 0.0 || y[2] != -20.0) return 2;
    if (info.rows_empty != 1 || info.rows_split != 0 || info.tiles != 1 || info.entries != 4) return 3;
    spECK::SpMV(A, static_cast<const double*>(dx.data), static_cast<double*>(dy.data), config, 2.0, -3.0);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 8) != SPECK_OK) return 1;
    if (y[0] != 5.0 || y[1] != 0.0 || y[2] != 20.0) return 4;
    speck_dcsr_free(&dx);
    speck_dcsr_free(&dy);
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "spmv caller ok\n" : "spmv caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("spmv caller: %s\n", e.what());
        return 100;
    }
}
