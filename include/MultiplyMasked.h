// MultiplyMasked.h -- spECK::MultiplyMasked: matOut = Mask o (A B), the product kept only where the mask has an entry
// (triangle counting, a Galerkin product kept on a known pattern, the gradient of a sparse product with respect to a
// sparse operand).  No reference counterpart.  Only the pattern of Mask is read.  Instantiated for float and double; see
// speck_multiply_masked_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void MultiplyMasked(const dCSR<DataType>& A, const dCSR<DataType>& B, const dCSR<DataType>& Mask, dCSR<DataType>& matOut,
                    spECKConfig& config, int flags = SPECK_MASK_STRUCTURE, speck_masked_info* info = nullptr)
{
    speck_dcsr a = A.raw(), b = B.raw(), m = Mask.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_multiply_masked_f64(config.handle, &a, &b, &m, &c, flags, info)
                                         : speck_multiply_masked_f32(config.handle, &a, &b, &m, &c, flags, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::MultiplyMasked: ") + speck_status_string(rc));
}
}  // namespace spECK
