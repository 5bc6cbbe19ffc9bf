// A caller that includes Semiring.h only: one Bellman-Ford step y = min(x, A (min,+) x) on a small matrix with an empty
// row, then the (max, second) block product with two right-hand sides in padded rows, in both precisions.  Without a
// device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_semiring.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Semiring.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 2 0; 0 0 0; 5 0 7]; x = [0 10 1]; the vectors and blocks travel as the data arrays of 1 x n matrices of doubles
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2}, ro3[2] = {0, 3}, ro9[2] = {0, 9}, ro12[2] = {0, 12};
    const unsigned ids[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const T v[4] = {1, 2, 5, 7};
    const double x[3] = {0, 10, 1}, y0[3] = {77, 77, 77};
    const double X[9] = {3, 1, 99, 4, 0, 99, 5, -1, 99};
    const double Y0[12] = {1, 1, 77, 77, 1, 1, 77, 77, 1, 1, 77, 77};
    speck_dcsr da{}, dx{}, dy{}, dX{}, dY{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dx, 1, 3, 3, ro3, ids, x, 8) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dy, 1, 3, 3, ro3, ids, y0, 8) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dX, 1, 9, 9, ro9, ids, X, 8) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&dY, 1, 12, 12, ro12, ids, Y0, 8) != SPECK_OK) return 1;
    dCSR<T> A;
    A.adopt(da);
    speck_semiring_info info{};
    double y[12];
    // z = x: min(0, min(1 + 0, 2 + 10)), min(10, +inf), min(1, min(5 + 0, 7 + 1))
    spECK::SpMVSemiring(A, SPECK_SR_MIN_PLUS, static_cast<const double*>(dx.data), static_cast<double*>(dy.data), config,
                        static_cast<const double*>(dx.data), &info);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 8) != SPECK_OK) return 1;
    if (y[0] != 0 || y[1] != 10 || y[2] != 1) return 2;
    if (info.rows_empty != 1 || info.rows_split != 0 || info.tiles != 1 || info.entries != 4 || info.terms != 4 || info.changed != 0) return 3;
    // no z: the sums themselves, the identity for the row without entries
    spECK::SpMVSemiring(A, SPECK_SR_MIN_PLUS, static_cast<const double*>(dx.data), static_cast<double*>(dy.data), config);
    if (speck_dcsr_download(&dy, nullptr, nullptr, y, 8) != SPECK_OK) return 1;
    if (y[0] != 1 || !(std::isinf(y[1]) && y[1] > 0) || y[2] != 5) return 4;
    // (max, second) on the block, in place on Y: max(1, max(3, 4)), max(1, max(1, 0)); 1, 1; max(1, max(3, 5)), max(1, max(1, -1))
    spECK::SpMMSemiring(A, SPECK_SR_MAX_SECOND, static_cast<const double*>(dX.data), 3, 2, static_cast<double*>(dY.data), 4, config,
                        static_cast<const double*>(dY.data), 4, &info);
    if (speck_dcsr_download(&dY, nullptr, nullptr, y, 8) != SPECK_OK) return 1;
    const double want[12] = {4, 1, 77, 77, 1, 1, 77, 77, 5, 1, 77, 77};
    for (int i = 0; i < 12; ++i)
        if (y[i] != want[i]) return 5;
    if (info.terms != 8 || info.changed != 2) return 6;
    speck_dcsr_free(&dx);
    speck_dcsr_free(&dy);
    speck_dcsr_free(&dX);
    speck_dcsr_free(&dY);
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "semiring caller ok\n" : "semiring caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("semiring caller: %s\n", e.what());
        return 100;
    }
}
