// A caller that includes Extract.h only: rows 2, 0, 2 of a 3 x 3 matrix with column 0 renamed 1, column 2 renamed 0 and
// column 1 dropped, in both precisions and with both index types.  Device arrays come from speck_dcsr_upload (ids as the
// col_ids of a matrix without rows, 8-byte ids as its values).  Without a device the config cannot be created and the
// caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_extract.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>

#include "Extract.h"

// n ids on the device: the col_ids (uint32_t) or the data (int64_t, as doubles bit for bit) of `hold`
template <typename I>
static const I* device_ids(dCSR<double>& hold, const int64_t* ids, unsigned n)
{
    const unsigned ro[1] = {0};
    unsigned narrow[8];
    double wide[8];
    for (unsigned i = 0; i < n; ++i) {
        narrow[i] = (unsigned)ids[i];
        std::memcpy(&wide[i], &ids[i], 8);
    }
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 0, 8, n, ro, narrow, wide, 8) != SPECK_OK) return nullptr;
    hold.adopt(d);
    return sizeof(I) == 8 ? reinterpret_cast<const I*>(hold.data) : reinterpret_cast<const I*>(hold.col_ids);
}

template <typename T, typename I>
static int one(spECK::spECKConfig& config)
{
    const unsigned a_ro[4] = {0, 2, 3, 6}, a_ci[6] = {0, 1, 2, 0, 1, 2};
    const T a_v[6] = {1, 2, 3, 4, 5, 6};
    const int64_t index[3] = {2, 0, 2}, map[3] = {1, -1, 0};
    dCSR<T> A, C;
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 3, 3, 6, a_ro, a_ci, a_v, sizeof(T)) != SPECK_OK) return 1;
    A.adopt(d);
    dCSR<double> hold_index, hold_map;
    const I* d_index = device_ids<I>(hold_index, index, 3);
    const I* d_map = device_ids<I>(hold_map, map, 3);
    if (!d_index || !d_map) return 1;
    speck_extract_info info{};
    spECK::Extract<T, I>(A, 3, d_index, 2, d_map, C, config, &info);
    if (C.rows != 3 || C.cols != 2 || C.nnz != 5 || info.rows_out != 3 || info.rows_empty != 0 || info.gross != 8 || info.nnz_out != 5 ||
        info.dropped != 3 || info.cols_kept != 2 || info.max_row_entries != 2)
        return 2;
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 2, 3, 5}, want_ci[5] = {1, 0, 1, 1, 0};
    const T want_v[5] = {4, 6, 1, 4, 6};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    // canonical: the rows sorted by their new ids
    dCSR<T> S;
    spECK::Extract<T, I>(A, 3, d_index, 2, d_map, S, config, nullptr, true);
    r = S.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    if (got_ci[0] != 0 || got_ci[1] != 1 || got_v[0] != 6 || got_v[1] != 4) return 7;
    // no index, no map: a copy
    dCSR<T> W;
    spECK::Extract<T, I>(A, 3, nullptr, 3, nullptr, W, config);
    if (W.rows != 3 || W.cols != 3 || W.nnz != 6) return 8;
    // an index beyond the rows is refused and leaves the result as it was
    const int64_t beyond[3] = {2, 3, 0};
    dCSR<double> hold_bad;
    const I* d_bad = device_ids<I>(hold_bad, beyond, 3);
    if (!d_bad) return 1;
    try {
        spECK::Extract<T, I>(A, 3, d_bad, 2, d_map, C, config);
        return 9;
    } catch (const std::runtime_error&) {
        if (C.rows != 3 || C.cols != 2 || C.nnz != 5) return 10;
    }
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double, uint32_t>(config) * 1000000 + one<float, uint32_t>(config) * 10000 + one<double, int64_t>(config) * 100 +
                       one<float, int64_t>(config);
        config.cleanup();
        std::printf(rc == 0 ? "extract caller ok\n" : "extract caller FAILED %d\n", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("extract caller: %s\n", e.what());
        return 100;
    }
}
