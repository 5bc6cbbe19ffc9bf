// A caller that includes FromCOO.h only: five unordered triplets grouped into a 3 x 3 matrix, in both precisions and with
// both index types, then expanded again.  Device arrays come from speck_dcsr_upload (ids as the col_ids of a matrix
// without rows, 8-byte ids as its values).  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_from_coo.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>

#include "FromCOO.h"

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
    const int64_t row[5] = {2, 0, 2, 1, 0}, col[5] = {1, 2, 0, 1, 0};
    const T val[5] = {1, 2, 3, 4, 5};
    dCSR<double> hold_row, hold_col;
    dCSR<T> hold_val, C;
    const I* d_row = device_ids<I>(hold_row, row, 5);
    const I* d_col = device_ids<I>(hold_col, col, 5);
    const unsigned ro0[1] = {0}, ci0[5] = {0, 0, 0, 0, 0};
    speck_dcsr d{};
    if (!d_row || !d_col || speck_dcsr_upload(&d, 0, 8, 5, ro0, ci0, val, sizeof(T)) != SPECK_OK) return 1;
    hold_val.adopt(d);
    speck_from_coo_info info{};
    spECK::FromCOO<T, I>(C, 3, 3, 5, d_row, d_col, hold_val.data, config, false, false, &info);
    if (C.rows != 3 || C.cols != 3 || C.nnz != 5 || info.entries != 5 || info.rows_empty != 0 || info.max_row_entries != 2 ||
        info.sorted_input != 0 || info.sort_passes != 1)
        return 2;
    unsigned got_ro[4], got_ci[5];
    T got_v[5];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 3;
    const unsigned want_ro[4] = {0, 2, 3, 5}, want_ci[5] = {2, 0, 1, 1, 0};
    const T want_v[5] = {2, 5, 4, 1, 3};
    for (int i = 0; i < 5; ++i)
        if (got_ci[i] != want_ci[i] || got_v[i] != want_v[i]) return 4;
    for (int i = 0; i < 4; ++i)
        if (got_ro[i] != want_ro[i]) return 5;
    // canonical: the rows sorted by column
    dCSR<T> S;
    spECK::FromCOO<T, I>(S, 3, 3, 5, d_row, d_col, hold_val.data, config, true);
    r = S.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got_v, sizeof(T)) != SPECK_OK) return 6;
    if (got_ci[0] != 0 || got_ci[1] != 2 || got_v[0] != 5 || got_v[1] != 2) return 7;
    // and back: the row of every entry, from row 10 on
    dCSR<double> out_row, out_col;
    const int64_t zeros[5] = {0, 0, 0, 0, 0};
    I* d_out_row = const_cast<I*>(device_ids<I>(out_row, zeros, 5));
    I* d_out_col = const_cast<I*>(device_ids<I>(out_col, zeros, 5));
    if (!d_out_row || !d_out_col) return 8;
    spECK::ToCOO<I>(C, d_out_row, d_out_col, config, 10);
    unsigned ci[5];
    double da[5];
    unsigned one_ro[1];
    int64_t got[2][5];
    dCSR<double>* outs[2] = {&out_row, &out_col};
    for (int k = 0; k < 2; ++k) {
        r = outs[k]->raw();
        if (speck_dcsr_download(&r, one_ro, ci, da, 8) != SPECK_OK) return 9;
        for (int i = 0; i < 5; ++i) {
            if (sizeof(I) == 8) std::memcpy(&got[k][i], &da[i], 8);
            else got[k][i] = ci[i];
        }
    }
    const int64_t want_row[5] = {10, 10, 11, 12, 12};
    for (int i = 0; i < 5; ++i)
        if (got[0][i] != want_row[i] || got[1][i] != (int64_t)want_ci[i]) return 10;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double, uint32_t>(config) * 1000000 + one<float, uint32_t>(config) * 10000 + one<double, int64_t>(config) * 100 +
                       one<float, int64_t>(config);
        config.cleanup();
        std::printf(rc == 0 ? "from_coo caller ok\n" : "from_coo caller FAILED %d\n", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("from_coo caller: %s\n", e.what());
        return 100;
    }
}
