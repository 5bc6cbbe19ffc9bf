// A caller that includes TopK.h only: the two best entries of every row of a 3 x 4 matrix, by value and by magnitude, in
// both precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_topk.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "TopK.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // row 0: 1 -5 3 3 (the tie: the first 3 wins); row 1: 7; row 2: -2 -1 -9
    const unsigned a_ro[4] = {0, 4, 5, 8}, a_ci[8] = {0, 1, 2, 3, 2, 0, 1, 3};
    const T a_v[8] = {1, -5, 3, 3, 7, -2, -1, -9};
    dCSR<T> A, C;
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 4, 8, a_ro, a_ci, a_v, sizeof(T)) != SPECK_OK) return 1;
    A.adopt(d);
    speck_topk_info info{};
    spECK::TopK<T>(A, 2, SPECK_TOPK_LARGEST, C, config, &info);
    if (C.rows != 3 || C.cols != 4 || C.nnz != 5 || info.rows != 3 || info.rows_cut != 2 || info.entries_in != 8 || info.nnz_out != 5 ||
        info.dropped != 3 || info.max_row_entries != 2 || info.ties_cut != 0 || info.nan_kept != 0)
        return 2;
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 2, 3, 5}, want_ci[5] = {2, 3, 2, 0, 1};
    const T want_v[5] = {3, 3, 7, -2, -1};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    // by magnitude: -5 and the first 3; 7; -2 and -9 -- the tie rule decided in row 0
    spECK::TopK<T>(A, 2, SPECK_TOPK_LARGEST_ABS, C, config, &info);
    r = C.raw();
    if (C.nnz != 5 || info.ties_cut != 1 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    const unsigned abs_ci[5] = {1, 2, 2, 0, 3};
    const T abs_v[5] = {-5, 3, 7, -2, -9};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != abs_ci[i] || got_v[i] != abs_v[i]) return 7;
    // a mode that does not exist is refused and leaves the result as it was
    try {
        spECK::TopK<T>(A, 2, 3, C, config);
        return 8;
    } catch (const std::runtime_error&) {
        if (C.rows != 3 || C.cols != 4 || C.nnz != 5) return 9;
    }
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 100 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "topk caller ok\n" : "topk caller FAILED %d\n", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("topk caller: %s\n", e.what());
        return 100;
    }
}
