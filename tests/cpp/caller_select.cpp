// A caller that includes Select.h only: the strict lower triangle of a small matrix, then its entries on the pattern of
// that triangle whose magnitude exceeds 3, in both precisions.  Without a device the config cannot be created and the
// caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_select.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Select.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // S = [1 2 0; 3 0 -4; 5 6 7]: strictly below the diagonal 3, 5, 6
    const unsigned ro[4] = {0, 2, 4, 7}, ci[7] = {0, 1, 0, 2, 0, 1, 2};
    const T v[7] = {1, 2, 3, -4, 5, 6, 7};
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 3, 7, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> S, L, C;
    S.adopt(d);
    speck_select_params p{};
    p.flags = SPECK_SELECT_BAND;
    p.band_lo = INT64_MIN, p.band_hi = -1;
    speck_select_info info{};
    spECK::Select(S, p, L, config, &info);
    if (L.nnz != 3 || info.kept != 3 || info.dropped != 4 || info.rows_unchanged != 0 || info.nnz_out != 3) return 2;
    unsigned got_ro[4], got_ci[3];
    T got_v[3];
    speck_dcsr r = L.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 0, 1, 3}, want_ci[3] = {0, 0, 1};
    const T want_v[3] = {3, 5, 6};
    for (int i = 0; i < 3; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    speck_dcsr l = L.raw();
    p = speck_select_params{};
    p.flags = SPECK_SELECT_PATTERN | SPECK_SELECT_ABS;
    p.abs_threshold = 3.0;
    p.pattern = &l;
    spECK::Select(S, p, C, config);
    r = C.raw();
    if (C.nnz != 2 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    if (got_ro[1] != 0 || got_ro[2] != 0 || got_ro[3] != 2 || got_ci[0] != 0 || got_ci[1] != 1 || got_v[0] != 5 || got_v[1] != 6)
        return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "select caller ok\n" : "select caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("select caller: %s\n", e.what());
        return 100;
    }
}
