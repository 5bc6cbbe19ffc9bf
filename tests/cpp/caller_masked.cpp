// A caller that includes MultiplyMasked.h only: the square of a small matrix kept on the matrix's own pattern, in both
// modes and both precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_masked.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdio>
#include <exception>

#include "MultiplyMasked.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // S = [1 2 0; 0 3 0; 4 0 5],  S S = [1 8 0; 0 9 0; 24 8 25]: on the pattern of S the entry (2,1) goes
    const unsigned ro[4] = {0, 2, 3, 5}, ci[5] = {0, 1, 1, 0, 2};
    const T v[5] = {1, 2, 3, 4, 5};
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 3, 5, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> S, C;
    S.adopt(d);
    speck_masked_info info{};
    spECK::MultiplyMasked(S, S, S, C, config, SPECK_MASK_STRUCTURE, &info);
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = C.raw();
    if (C.nnz != 5 || info.nnz_out != 5 || info.products != 8 || info.hits != 7) return 2;
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const T want[5] = {1, 8, 9, 24, 25};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != ci[i] || got_v[i] != want[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != ro[i]) return 5;
    spECK::MultiplyMasked(S, S, S, C, config, SPECK_MASK_FULL_PATTERN);
    r = C.raw();
    if (C.nnz != 5 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != ci[i] || got_v[i] != want[i]) return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "masked caller ok\n" : "masked caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("masked caller: %s\n", e.what());
        return 100;
    }
}
