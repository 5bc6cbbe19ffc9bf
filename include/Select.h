// Select.h -- spECK::Select: matOut = the entries of A that every selected predicate keeps (a diagonal band, a magnitude,
// membership in the pattern of another matrix; each may be negated), in input order, bit for bit -- tril / triu of a matrix
// that is already on the device, "keep (i,j) in M" behind a product, explicit zeros dropped.  No reference counterpart.
// Instantiated for float and double; see speck_select_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void Select(const dCSR<DataType>& A, const speck_select_params& params, dCSR<DataType>& matOut, spECKConfig& config,
            speck_select_info* info = nullptr)
{
    speck_dcsr a = A.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_select_f64(config.handle, &a, &params, &c, info)
                                         : speck_select_f32(config.handle, &a, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Select: ") + speck_status_string(rc));
}
}  // namespace spECK
