// A caller that includes Sample.h only: two neighbours per row of a 3 x 4 matrix without replacement, then two draws with
// replacement for the rows a device index list names (the column ids of a one-row matrix: a vertex's neighbour list is
// the next frontier), in both precisions.  The expectations are tests/test_sample_host.py's numpy statement (which checks
// this file against itself).  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_sample.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Sample.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // row 0: 1 -5 3 3; row 1: 7; row 2: -2 -1 -9
    const unsigned a_ro[4] = {0, 4, 5, 8}, a_ci[8] = {0, 1, 2, 3, 2, 0, 1, 3};
    const T a_v[8] = {1, -5, 3, 3, 7, -2, -1, -9};
    dCSR<T> A, C, F;
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 4, 8, a_ro, a_ci, a_v, sizeof(T)) != SPECK_OK) return 1;
    A.adopt(d);
    speck_sample_info info{};
    spECK::Sample<T>(A, 2, 1, SPECK_SAMPLE_WITHOUT_REPLACEMENT, C, config, nullptr, 0, 8, 0, &info);
    if (C.rows != 3 || C.cols != 4 || C.nnz != 5 || info.rows_out != 3 || info.rows_empty != 0 || info.rows_cut != 2 || info.gross != 8 ||
        info.nnz_out != 5 || info.max_row_entries != 2)
        return 2;
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 2, 3, 5}, want_ci[5] = {0, 2, 2, 0, 1};
    const T want_v[5] = {1, 3, 7, -2, -1};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    // the frontier 2, 0 as the ids of a one-row matrix; two draws each, in draw order
    const unsigned f_ro[2] = {0, 2}, f_ci[2] = {2, 0};
    const T f_v[2] = {1, 1};
    speck_dcsr f{};
    if (speck_dcsr_upload(&f, 1, 4, 2, f_ro, f_ci, f_v, sizeof(T)) != SPECK_OK) return 6;
    F.adopt(f);
    spECK::Sample<T>(A, 2, 1, SPECK_SAMPLE_WITH_REPLACEMENT, C, config, F.raw().col_ids, 2, 4, 0, &info);
    r = C.raw();
    if (C.rows != 2 || C.cols != 4 || C.nnz != 4 || info.rows_cut != 2 || info.gross != 7 ||
        speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK)
        return 7;
    const unsigned draw_ro[3] = {0, 2, 4}, draw_ci[4] = {1, 1, 1, 3};
    const T draw_v[4] = {-1, -1, -5, 3};
    for (int i = 0; i < 4; ++i)
        if (got_ci[i] != draw_ci[i] || got_v[i] != draw_v[i]) return 8;
    for (int i = 0; i < 3; ++i)
        if (got_ro[i] != draw_ro[i]) return 9;
    // a mode that does not exist is refused and leaves the result as it was
    try {
        spECK::Sample<T>(A, 2, 1, 2, C, config);
        return 10;
    } catch (const std::runtime_error&) {
        if (C.rows != 2 || C.cols != 4 || C.nnz != 4) return 11;
    }
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 100 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "sample caller ok\n" : "sample caller FAILED %d\n", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("sample caller: %s\n", e.what());
        return 100;
    }
}
