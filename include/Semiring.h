// Semiring.h -- spECK::SpMVSemiring, spECK::SpMMSemiring: y = [z (+)] A (x) x on a device matrix over one of the semirings
// SPECK_SR_* -- (+) is min or max, (x) is a + x[j], a * x[j] or x[j] alone (SECOND: A's values are never read).  Vectors
// and row-major blocks of doubles for both value types as spECK::SpMV and spECK::SpMM take them; d_z may be null (y = s),
// may be d_x, or may be d_y itself (for blocks with ldz == ldy: in place).  A row without entries gives the identity, +inf
// or -inf.  min and max are exact and propagate a NaN: the same values from run to run, on a row-range view and for every
// k.  info->changed counts the elements of y that differ from z: what ends a relaxation loop.  No reference counterpart.
// Instantiated for float and double; see speck_spmv_sr_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void SpMVSemiring(const dCSR<DataType>& A, int semiring, const double* d_x, double* d_y, spECKConfig& config,
                  const double* d_z = nullptr, speck_semiring_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmv_sr_f64(config.handle, semiring, &a, d_x, d_z, d_y, info)
                                         : speck_spmv_sr_f32(config.handle, semiring, &a, d_x, d_z, d_y, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMVSemiring: ") + speck_status_string(rc));
}

template <typename DataType>
void SpMMSemiring(const dCSR<DataType>& A, int semiring, const double* d_X, uint64_t ldx, uint32_t k, double* d_Y, uint64_t ldy,
                  spECKConfig& config, const double* d_Z = nullptr, uint64_t ldz = 0, speck_semiring_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmm_sr_f64(config.handle, semiring, &a, d_X, ldx, k, d_Z, ldz, d_Y, ldy, info)
                                         : speck_spmm_sr_f32(config.handle, semiring, &a, d_X, ldx, k, d_Z, ldz, d_Y, ldy, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMMSemiring: ") + speck_status_string(rc));
}
}  // namespace spECK
