// A caller that includes Softmax.h only: the row softmax of a small matrix into a new matrix, then its backward in
// place, in both precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_softmax.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <exception>

#include "Softmax.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [0 0 .; . . .; 3 . 3]: every row with entries holds two equal ones, so p = 1/2 exactly
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2};
    const T v[4] = {0, 0, 3, 3};
    speck_dcsr da{}, dg{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    const T gv[4] = {1, 3, -2, 2};
    if (speck_dcsr_upload(&dg, 3, 3, 4, ro, ci, gv, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> A, G, P;
    A.adopt(da);
    G.adopt(dg);
    speck_softmax_info info{};
    spECK::Softmax(A, config, 1.0, &P, SPECK_SOFTMAX_NORMALIZED, nullptr, nullptr, &info);
    if (P.rows != 3 || P.nnz != 4 || info.entries != 4 || info.nonfinite != 0 || info.rows_empty != 1 || info.rows_split != 0 ||
        info.tiles != 1)
        return 2;
    unsigned got_ro[4], got_ci[4];
    T got[4];
    speck_dcsr r = P.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 3;
    for (int i = 0; i < 4; ++i)
        if (got[i] != T(0.5) || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 4;
    // in place: 2 p (g - r), r = (1 + 3) / 2 = 2 and (-2 + 2) / 2 = 0
    spECK::SoftmaxBackward(P, G, config, 2.0, static_cast<dCSR<T>*>(nullptr), nullptr, &info);
    if (info.entries != 4 || info.nonfinite != 0) return 5;
    r = P.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 6;
    const T want[4] = {-1, 1, -2, 2};
    for (int i = 0; i < 4; ++i)
        if (got[i] != want[i] || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "softmax caller ok\n" : "softmax caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("softmax caller: %s\n", e.what());
        return 100;
    }
}
