// A caller that includes Add.h only: 2 A - B of two small matrices whose patterns overlap in part, then A - A, in both
// precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_add.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Add.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 2 0; 0 0 0; 5 0 7], B = [0 4 8; 0 3 0; 5 0 0]
    const unsigned a_ro[4] = {0, 2, 2, 4}, a_ci[4] = {0, 1, 0, 2};
    const T a_v[4] = {1, 2, 5, 7};
    const unsigned b_ro[4] = {0, 2, 3, 4}, b_ci[4] = {1, 2, 1, 0};
    const T b_v[4] = {4, 8, 3, 5};
    speck_dcsr da{}, db{};
    if (speck_dcsr_upload(&da, 3, 3, 4, a_ro, a_ci, a_v, sizeof(T)) != SPECK_OK) return 1;
    if (speck_dcsr_upload(&db, 3, 3, 4, b_ro, b_ci, b_v, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> A, B, C;
    A.adopt(da);
    B.adopt(db);
    speck_add_info info{};
    spECK::Add(2.0, A, -1.0, B, C, config, &info);
    if (C.nnz != 6 || info.only_a != 2 || info.only_b != 2 || info.both != 2 || info.nnz_out != 6) return 2;
    unsigned got_ro[4], got_ci[6];
    T got_v[6];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 3, 4, 6}, want_ci[6] = {0, 1, 2, 1, 0, 2};
    const T want_v[6] = {2, 0, -8, -3, 5, 14};
    for (int i = 0; i < 6; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    spECK::Add(1.0, A, -1.0, A, C, config);  // the same matrix twice: every entry stays, as +0.0
    r = C.raw();
    if (C.nnz != 4 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    for (int i = 0; i < 4; ++i)
        if (got_ci[i] != a_ci[i] || got_v[i] != 0) return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "add caller ok\n" : "add caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("add caller: %s\n", e.what());
        return 100;
    }
}
