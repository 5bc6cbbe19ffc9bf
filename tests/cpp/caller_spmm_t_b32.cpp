// A caller that includes SpMMT.h only and passes FLOAT blocks: Y = A^T X and Y = 2 A^T X - 3 Y of a small 3 x 4 matrix with
// an empty column and two right-hand sides in padded rows (ldx = 3, ldy = 4, counted in floats), in both value types of A,
// through ONE plan; then the plan against a matrix with another pattern, which is refused.  Without a device the config
// cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_spmm_t_b32.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "SpMMT.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -2 0 0; 0 0 0 0; 5 0 0 -7] (column 2 is empty), X = [3 1; 4 0; 5 -1] with one word of padding per row, Y (4 x 2)
    // with two; the blocks travel as the data arrays of two 1 x n matrices of floats
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 3}, other[4] = {0, 1, 1, 3}, xro[2] = {0, 9}, yro[2] = {0, 16};
    const unsigned ids[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const T v[4] = {1, -2, 5, -7};
    const float x[9] = {3, 1, 99, 4, 0, 99, 5, -1, 99};
    const float y0[16] = {1, 1, 77, 77, 1, 1, 77, 77, 1, 1, 77, 77, 1, 1, 77, 77};
    speck_dcsr da{}, db{}, dx{}, dy{};
    if (speck_dcsr_upload(&da, 3, 4, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&db, 3, 4, 4, ro, other, v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dx, 1, 9, 9, xro, ids, x, 4) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dy, 1, 16, 16, yro, ids, y0, 4) != SPECK_OK) return 1;
    dCSR<T> A, B;
    A.adopt(da);
    B.adopt(db);
    spECK::TransposePlan plan(A);
    if (!plan) return 5;
    speck_spmm_t_info info{};
    float y[16];
    spECK::SpMMT(plan, A, static_cast<const float*>(dx.data), 3, 2, static_cast<float*>(dy.data), 4, config, 1.0, 0.0, &info);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 4) != SPECK_OK) return 1;
    // A^T X: column 0 = 1 X(0,:) + 5 X(2,:), column 1 = -2 X(0,:), column 2 empty, column 3 = -7 X(2,:)
    const float want[16] = {28, -4, 77, 77, -6, -2, 77, 77, 0, 0, 77, 77, -35, 7, 77, 77};
    for (int i = 0; i < 16; ++i)
        if (y[i] != want[i]) return 2;
    if (info.cols_empty != 1 || info.cols_split != 0 || info.tiles != 1 || info.entries != 4 || info.terms != 8) return 3;
    spECK::SpMMT(plan, A, static_cast<const float*>(dx.data), 3, 2, static_cast<float*>(dy.data), 4, config, 2.0, -3.0);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 4) != SPECK_OK) return 1;
    const float then[16] = {-28, 4, 77, 77, 6, 2, 77, 77, 0, 0, 77, 77, 35, -7, 77, 77};
    for (int i = 0; i < 16; ++i)
        if (y[i] != then[i]) return 4;
    // the same shape and nnz, another pattern: refused, and Y keeps what it held
    bool refused = false;
    try {
        spECK::SpMMT(plan, B, static_cast<const float*>(dx.data), 3, 2, static_cast<float*>(dy.data), 4, config);
    } catch (const std::exception&) {
        refused = true;
    }
    if (!refused) return 6;
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 4) != SPECK_OK) return 1;
    for (int i = 0; i < 16; ++i)
        if (y[i] != then[i]) return 7;
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
        std::printf(rc == 0 ? "spmm_t_b32 caller ok\n" : "spmm_t_b32 caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("spmm_t_b32 caller: %s\n", e.what());
        return 100;
    }
}
