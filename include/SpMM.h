// SpMM.h -- spECK::SpMM: Y = alpha A X + beta Y on a device matrix with k right-hand sides; d_X (A.cols x k) and d_Y
// (A.rows x k, indexed by the row inside A) are ROW-MAJOR device arrays of doubles for both value types, with leading
// dimensions ldx >= k and ldy >= k (a contiguous torch tensor, or a column slice of one).  A is read once for all k
// columns; column c of Y is bit for bit what spECK::SpMV writes for X(:,c) and Y(:,c): the same bits from run to run, a
// row-range view gives the rows of the whole result, beta == 0 does not read Y, a NaN is never hidden.  The padding of a
// row of Y is neither read nor written.  No reference counterpart.
// Instantiated for float and double; see speck_spmm_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void SpMM(const dCSR<DataType>& A, const double* d_X, uint64_t ldx, uint32_t k, double* d_Y, uint64_t ldy, spECKConfig& config,
          double alpha = 1.0, double beta = 0.0, speck_spmm_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmm_f64(config.handle, alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info)
                                         : speck_spmm_f32(config.handle, alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMM: ") + speck_status_string(rc));
}

// float blocks (speck_spmm_f64_b32 / _f32_b32): ldx and ldy count floats; Y is bit for bit the result above on the widened
// blocks, rounded to float once
template <typename DataType>
void SpMM(const dCSR<DataType>& A, const float* d_X, uint64_t ldx, uint32_t k, float* d_Y, uint64_t ldy, spECKConfig& config,
          double alpha = 1.0, double beta = 0.0, speck_spmm_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmm_f64_b32(config.handle, alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info)
                                         : speck_spmm_f32_b32(config.handle, alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMM: ") + speck_status_string(rc));
}
}  // namespace spECK
