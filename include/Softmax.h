// Softmax.h -- spECK::Softmax: the softmax of every row of a device matrix over the entries the row holds, p = exp(alpha a
// - m_i) / s_i (SPECK_SOFTMAX_EXP: without the division), and spECK::SoftmaxBackward: alpha p (g - r_i) with r_i the row's
// sum of p g, G a matrix with P's pattern.  C == nullptr works in place.  d_row_max / d_row_sum (device, A.rows doubles,
// optional) receive m_i and s_i (backward: r_i).  Every step in double, the row sums in the tree of spECK::Reduce: the
// same bits from run to run, in place or not, on a row-range view as on the whole matrix; a -inf entry is a mask, a NaN
// or +inf is never hidden.  The step between spECK::SDDMM and spECK::SpMM of an attention layer.  No reference counterpart.
// Not built: log_softmax, a column softmax (Transpose first), the softmax fused into SDDMM or SpMM, float vectors, a
// per-row temperature, a pattern check of G.
// Instantiated for float and double; see speck_softmax_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void Softmax(const dCSR<DataType>& A, spECKConfig& config, double alpha = 1.0, dCSR<DataType>* C = nullptr,
             int mode = SPECK_SOFTMAX_NORMALIZED, double* d_row_max = nullptr, double* d_row_sum = nullptr,
             speck_softmax_info* info = nullptr, const DataType* d_G = nullptr)
{
    speck_dcsr a = A.raw();
    speck_softmax_params p{};
    p.mode = (uint32_t)mode, p.alpha = alpha;
    p.d_G = d_G, p.d_row_max = d_row_max, p.d_row_sum = d_row_sum;
    speck_dcsr c{};
    if (C) c = C->raw();
    const int rc = sizeof(DataType) == 8 ? speck_softmax_f64(config.handle, &a, &p, C ? &c : nullptr, info)
                                         : speck_softmax_f32(config.handle, &a, &p, C ? &c : nullptr, info);
    if (C) C->adopt(c);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Softmax: ") + speck_status_string(rc));
}

// P: the forward result; G: the gradient with respect to it, a matrix with P's pattern (its data laid out as P's: for a
// row-range view of P, the same view of G's owner)
template <typename DataType>
void SoftmaxBackward(const dCSR<DataType>& P, const dCSR<DataType>& G, spECKConfig& config, double alpha = 1.0,
                     dCSR<DataType>* C = nullptr, double* d_row_sum = nullptr, speck_softmax_info* info = nullptr)
{
    if (G.rows != P.rows || G.nnz != P.nnz) throw std::runtime_error("spECK::SoftmaxBackward: G must have P's pattern");
    Softmax(P, config, alpha, C, SPECK_SOFTMAX_BACKWARD, nullptr, d_row_sum, info, G.data);
}
}  // namespace spECK
