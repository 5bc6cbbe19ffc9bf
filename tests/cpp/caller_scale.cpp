// A caller that includes Scale.h only: the rows of a small matrix divided by their absolute sums into a new matrix, then
// its squares scaled by a vector on both sides in place, in both precisions.  Without a device the config cannot be
// created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_scale.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Scale.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -3 0; 0 0 0; 2 0 -6], |row sums| 4, (none), 8
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2};
    const T v[4] = {1, -3, 2, -6};
    speck_dcsr da{}, dv{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    // (a device vector: the values of a matrix of one row)
    const unsigned vro[2] = {0, 3}, vci[3] = {0, 1, 2};
    const double sums[3] = {4, 1, 8};
    if (speck_dcsr_upload(&dv, 1, 3, 3, vro, vci, sums, sizeof(double)) != SPECK_OK) return 1;
    dCSR<T> A, C;
    dCSR<double> V;
    A.adopt(da);
    V.adopt(dv);
    speck_scale_params p{};
    p.alpha = 1.0;
    p.row_mode = SPECK_SCALE_DIV;
    p.d_row = V.data;
    speck_scale_info info{};
    spECK::Scale(A, p, C, config, &info);
    if (C.rows != 3 || C.nnz != 4 || info.entries != 4 || info.nonfinite != 0 || info.tiles != 1) return 2;
    unsigned got_ro[4], got_ci[4];
    T got[4];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 3;
    const T want[4] = {T(0.25), T(-0.75), T(0.25), T(-0.75)};
    for (int i = 0; i < 4; ++i)
        if (got[i] != want[i] || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 4;
    // in place: 0.5 v v l[i] l[j]
    p = speck_scale_params{};
    p.map = SPECK_MAP_SQUARE;
    p.alpha = 0.5;
    p.row_mode = p.col_mode = SPECK_SCALE_MUL;
    p.d_row = p.d_col = V.data;
    spECK::Scale(A, p, config, &info);
    if (A.nnz != 4 || info.entries != 4 || info.nonfinite != 0) return 5;
    r = A.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 6;
    const T want2[4] = {T(0.5 * 1 * 4 * 4), T(0.5 * 9 * 4 * 1), T(0.5 * 4 * 8 * 4), T(0.5 * 36 * 8 * 8)};
    for (int i = 0; i < 4; ++i)
        if (got[i] != want2[i] || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "scale caller ok\n" : "scale caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("scale caller: %s\n", e.what());
        return 100;
    }
}
