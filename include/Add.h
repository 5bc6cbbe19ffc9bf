// Add.h -- spECK::Add: matOut = alpha A + beta B on the union of the two patterns, rows ascending, every value computed in
// double and rounded once -- S + S^T, a product accumulated onto an earlier one, the difference of two results, a scaling.
// An entry that cancels to 0.0 stays.  No reference counterpart.
// Instantiated for float and double; see speck_add_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void Add(double alpha, const dCSR<DataType>& A, double beta, const dCSR<DataType>& B, dCSR<DataType>& matOut,
         spECKConfig& config, speck_add_info* info = nullptr)
{
    speck_dcsr a = A.raw(), b = B.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_add_f64(config.handle, alpha, &a, beta, &b, &c, SPECK_ADD_UNION, info)
                                         : speck_add_f32(config.handle, alpha, &a, beta, &b, &c, SPECK_ADD_UNION, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Add: ") + speck_status_string(rc));
}
}  // namespace spECK
