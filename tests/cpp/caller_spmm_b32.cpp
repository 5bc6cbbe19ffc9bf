// A caller that includes SpMM.h only and passes FLOAT blocks: Y = A X and Y = 2 A X - 3 Y of a small matrix with an empty
// row and two right-hand sides in padded rows (ldx = 3, ldy = 4, counted in floats), in both value types of A.  Without
// a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_spmm_b32.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "SpMM.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -2 0; 0 0 0; 5 0 -7], X = [3 1; 4 0; 5 -1] with one word of padding per row, Y with two; the blocks travel as
    // the data arrays of two 1 x n matrices of floats
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2}, xro[2] = {0, 9}, yro[2] = {0, 12};
    const unsigned ids[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const T v[4] = {1, -2, 5, -7};
    const float x[9] = {3, 1, 99, 4, 0, 99, 5, -1, 99};
    const float y0[12] = {1, 1, 77, 77, 1, 1, 77, 77, 1, 1, 77, 77};
    speck_dcsr da{}, dx{}, dy{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dx, 1, 9, 9, xro, ids, x, 4) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dy, 1, 12, 12, yro, ids, y0, 4) != SPECK_OK) return 1;
    dCSR<T> A;
    A.adopt(da);
    speck_spmm_info info{};
    float y[12];
    spECK::SpMM(A, static_cast<const float*>(dx.data), 3, 2, static_cast<float*>(dy.data), 4, config, 1.0, 0.0, &info);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 4) != SPECK_OK) return 1;
    const float want[12] = {-5, 1, 77, 77, 0, 0, 77, 77, -20, 12, 77, 77};
    for (int i = 0; i < 12; ++i)
        if (y[i] != want[i]) return 2;
    if (info.rows_empty != 1 || info.rows_split != 0 || info.tiles != 1 || info.entries != 4 || info.terms != 8) return 3;
    spECK::SpMM(A, static_cast<const float*>(dx.data), 3, 2, static_cast<float*>(dy.data), 4, config, 2.0, -3.0);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 4) != SPECK_OK) return 1;
    const float then[12] = {5, -1, 77, 77, 0, 0, 77, 77, 20, -12, 77, 77};
    for (int i = 0; i < 12; ++i)
        if (y[i] != then[i]) return 4;
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
        std::printf(rc == 0 ? "spmm_b32 caller ok\n" : "spmm_b32 caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("spmm_b32 caller: %s\n", e.what());
        return 100;
    }
}
