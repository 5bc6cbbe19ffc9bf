// SDDMM.h -- spECK::SDDMM: C = alpha (U V^T) on A's pattern + beta A (or times A: SPECK_SDDMM_HADAMARD), the sampled
// dense-dense product on a device matrix; d_U (A.rows x k, indexed by the row inside A) and d_V (A.cols x k, indexed by the
// column id) are ROW-MAJOR device arrays of doubles for both value types, with leading dimensions ldu >= k and ldv >= k.
// C == nullptr works in place.  The sum over k runs in a tree that is a function of k alone: the same bits from run to
// run, in place or not, whatever the leading dimensions; beta == 0 does not read A's values; a NaN is never hidden.  The
// backward pass of spECK::SpMM with respect to A's values.  No reference counterpart.
// Instantiated for float and double; see speck_sddmm_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void SDDMM(const dCSR<DataType>& A, const double* d_U, uint64_t ldu, const double* d_V, uint64_t ldv, uint32_t k, spECKConfig& config,
           double alpha = 1.0, double beta = 0.0, dCSR<DataType>* C = nullptr, int mode = SPECK_SDDMM_AXPBY,
           speck_sddmm_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    speck_sddmm_params p{};
    p.mode = (uint32_t)mode, p.k = k, p.alpha = alpha, p.beta = beta;
    p.d_U = d_U, p.ldu = ldu, p.d_V = d_V, p.ldv = ldv;
    speck_dcsr c{};
    if (C) c = C->raw();
    const int rc = sizeof(DataType) == 8 ? speck_sddmm_f64(config.handle, &a, &p, C ? &c : nullptr, info)
                                         : speck_sddmm_f32(config.handle, &a, &p, C ? &c : nullptr, info);
    if (C) C->adopt(c);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SDDMM: ") + speck_status_string(rc));
}

// float blocks (speck_sddmm_f64_b32 / _f32_b32): ldu and ldv count floats; C is bit for bit the result above on the widened
// blocks
template <typename DataType>
void SDDMM(const dCSR<DataType>& A, const float* d_U, uint64_t ldu, const float* d_V, uint64_t ldv, uint32_t k, spECKConfig& config,
           double alpha = 1.0, double beta = 0.0, dCSR<DataType>* C = nullptr, int mode = SPECK_SDDMM_AXPBY,
           speck_sddmm_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    speck_sddmm_params_b32 p{};
    p.mode = (uint32_t)mode, p.k = k, p.alpha = alpha, p.beta = beta;
    p.d_U = d_U, p.ldu = ldu, p.d_V = d_V, p.ldv = ldv;
    speck_dcsr c{};
    if (C) c = C->raw();
    const int rc = sizeof(DataType) == 8 ? speck_sddmm_f64_b32(config.handle, &a, &p, C ? &c : nullptr, info)
                                         : speck_sddmm_f32_b32(config.handle, &a, &p, C ? &c : nullptr, info);
    if (C) C->adopt(c);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SDDMM: ") + speck_status_string(rc));
}
}  // namespace spECK
