// A caller that includes SDDMM.h only and passes FLOAT blocks: U V^T sampled on the pattern of a small matrix into a new
// matrix, then the residual A - U V^T in place, in both value types of A.  Without a device the config cannot be created
// and the caller says so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include tests/cpp/caller_sddmm_b32.cpp \
//       -Lspeck_amd -lspeck_amd -L/opt/rocm/lib -lamdhip64
#include <cstdint>
#include <cstdio>
#include <exception>

#include "SDDMM.h"

template <typename T>
static int one(spECK::spECKConfig& config)
{
    // A = [1 -3 0; 0 0 0; 2 0 -6]
    const unsigned ro[4] = {0, 2, 2, 4}, ci[4] = {0, 1, 0, 2};
    const T v[4] = {1, -3, 2, -6};
    speck_dcsr da{}, db{};
    if (speck_dcsr_upload(&da, 3, 3, 4, ro, ci, v, sizeof(T)) != SPECK_OK) return 1;
    // (a device block: the values of a matrix of one row) U = V = [1 2; 3 4; 5 6]
    const unsigned bro[2] = {0, 6}, bci[6] = {0, 1, 2, 3, 4, 5};
    const float block[6] = {1, 2, 3, 4, 5, 6};
    if (speck_dcsr_upload(&db, 1, 6, 6, bro, bci, block, sizeof(float)) != SPECK_OK) return 1;
    dCSR<T> A, C;
    dCSR<float> B;
    A.adopt(da);
    B.adopt(db);
    speck_sddmm_info info{};
    spECK::SDDMM(A, B.data, 2, B.data, 2, 2, config, 1.0, 0.0, &C, SPECK_SDDMM_AXPBY, &info);
    if (C.rows != 3 || C.nnz != 4 || info.entries != 4 || info.terms != 8 || info.nonfinite != 0 || info.tiles != 1 || info.lanes != 1)
        return 2;
    unsigned got_ro[4], got_ci[4];
    T got[4];
    speck_dcsr r = C.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 3;
    const T gram[4] = {5, 11, 17, 61};  // u0.u0, u0.u1, u2.u0, u2.u2
    for (int i = 0; i < 4; ++i)
        if (got[i] != gram[i] || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 4;
    // in place: A - U V^T
    spECK::SDDMM(A, B.data, 2, B.data, 2, 2, config, -1.0, 1.0, static_cast<dCSR<T>*>(nullptr), SPECK_SDDMM_AXPBY, &info);
    if (A.nnz != 4 || info.entries != 4 || info.nonfinite != 0) return 5;
    r = A.raw();
    if (speck_dcsr_download(&r, got_ro, got_ci, got, sizeof(T)) != SPECK_OK) return 6;
    for (int i = 0; i < 4; ++i)
        if (got[i] != v[i] - gram[i] || got_ci[i] != ci[i] || got_ro[i] != ro[i]) return 7;
    return 0;
}

int main()
{
    try {
        spECK::spECKConfig config = spECK::spECKConfig::initialize(0);
        const int rc = one<double>(config) * 10 + one<float>(config);
        config.cleanup();
        std::printf(rc == 0 ? "sddmm_b32 caller ok\n" : "sddmm_b32 caller FAILED %d\n", rc);
        return rc;
    } catch (const std::exception& e) {
        std::printf("sddmm_b32 caller: %s\n", e.what());
        return 100;
    }
}
