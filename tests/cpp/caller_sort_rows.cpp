// A caller that includes SortRows.h only: sorts a small matrix with an unsorted row and a duplicate, keeps the duplicate
// in the first pass and sums it in the second.  Without a device the call throws (the library reports the status).
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_sort_rows.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdio>
#include <exception>

#include "SortRows.h"

template <typename T>
static int one()
{
    // rows: [2:1, 0:2, 2:4] [] [1:8, 0:16]
    const unsigned ro[4] = {0, 3, 3, 5}, ci[5] = {2, 0, 2, 1, 0};
    const T v[5] = {1, 2, 4, 8, 16};
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 3, 5, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    dCSR<T> m;
    m.adopt(d);
    spECK::SortRows(m);
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = m.raw();
    if (m.nnz != 5 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 2;
    const unsigned want_ci[5] = {0, 2, 2, 0, 1};
    const T want_v[5] = {2, 1, 4, 16, 8};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 3;
    spECK::SortRows(m, true);
    r = m.raw();
    if (m.nnz != 4 || speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 4;
    const unsigned sum_ro[4] = {0, 2, 2, 4}, sum_ci[4] = {0, 2, 0, 1};
    const T sum_v[4] = {2, 5, 16, 8};
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != sum_ro[i] || got_ci[i] != sum_ci[i] || got_v[i] != sum_v[i]) return 5;
    return 0;
}

int main()
{
    try {
        const int rc = one<double>() * 10 + one<float>();
        std::printf(rc == 0 ? "sort-rows caller ok\n" : "sort-rows caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("sort-rows caller: %s\n", e.what());
        return 100;
    }
}
