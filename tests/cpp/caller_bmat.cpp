// A caller that includes BMat.h only: two small matrices stacked, joined, put on the diagonal and into a 2 x 2 grid with an
// empty block row, in both precisions.  Without a device the config cannot be created and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_bmat.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>
#include <vector>

#include "BMat.h"

template <typename T>
static bool holds(const dCSR<T>& C, size_t rows, size_t cols, const std::vector<unsigned>& ro, const std::vector<unsigned>& ci,
                  const std::vector<T>& v)
{
    if (C.rows != rows || C.cols != cols || C.nnz != ci.size()) return false;
    std::vector<unsigned> got_ro(rows + 1), got_ci(ci.size() + 1);
    std::vector<T> got_v(ci.size() + 1);
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro.data(), got_ci.data(), got_v.data(), sizeof(T)) != SPECK_OK) return false;
    for (size_t i = 0; i <= rows; ++i)
        if (got_ro[i] != ro[i]) return false;
    for (size_t i = 0; i < ci.size(); ++i)
        if (got_ci[i] != ci[i] || got_v[i] != v[i]) return false;
    return true;
}

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A: 2 x 3 = [[1 . 2], [. 3 .]];  B: 2 x 2 = [[. 4], [5 6]] with the last row unsorted (ids 1, 0)
    const unsigned a_ro[3] = {0, 2, 3}, a_ci[3] = {0, 2, 1}, b_ro[3] = {0, 1, 3}, b_ci[3] = {1, 1, 0};
    const T a_v[3] = {1, 2, 3}, b_v[3] = {4, 6, 5};
    dCSR<T> A, B, C;
    speck_dcsr d{};
    if (speck_dcsr_upload(&d, 2, 3, 3, a_ro, a_ci, a_v, sizeof(T)) != SPECK_OK) return 1;
    A.adopt(d);
    d = speck_dcsr{};
    if (speck_dcsr_upload(&d, 2, 2, 3, b_ro, b_ci, b_v, sizeof(T)) != SPECK_OK) return 1;
    B.adopt(d);
    speck_bmat_info info{};
    spECK::HStack<T>({&A, &B}, C, config, &info);
    if (!holds<T>(C, 2, 5, {0, 3, 6}, {0, 2, 4, 1, 4, 3}, {1, 2, 4, 3, 6, 5})) return 2;
    if (info.blocks != 2 || info.rows_out != 2 || info.cols_out != 5 || info.nnz_out != 6 || info.pieces != 4 || info.rows_empty != 0 ||
        info.max_row_entries != 3)
        return 3;
    spECK::BlockDiag<T>({&A, &B}, C, config);
    if (!holds<T>(C, 4, 5, {0, 2, 3, 4, 6}, {0, 2, 1, 4, 4, 3}, {1, 2, 3, 4, 6, 5})) return 4;
    spECK::VStack<T>({&A, &A}, C, config);  // one matrix in two cells
    if (!holds<T>(C, 4, 3, {0, 2, 3, 5, 6}, {0, 2, 1, 0, 2, 1}, {1, 2, 3, 1, 2, 3})) return 5;
    // [[B, A], [0, 0]] with an empty block row of 3
    spECK::BMat<T>({{0, 1, &A}, {0, 0, &B}}, 2, 2, C, config, {2, 3}, {2, 3});
    if (!holds<T>(C, 5, 5, {0, 3, 6, 6, 6, 6}, {1, 2, 4, 1, 0, 3}, {4, 1, 2, 6, 5, 3})) return 6;
    // blocks of different widths cannot be stacked: refused, the result stays
    try {
        spECK::VStack<T>({&A, &B}, C, config);
        return 7;
    } catch (const std::runtime_error&) {
        if (C.rows != 5 || C.cols != 5 || C.nnz != 6) return 8;
    }
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 100 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "bmat caller ok\n" : "bmat caller FAILED %d\n", rc);
        return rc ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("bmat caller: %s\n", e.what());
        return 100;
    }
}
