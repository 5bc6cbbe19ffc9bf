// Scale.h -- spECK::Scale: C(i,j) = ((alpha g(A(i,j))) (.) l[i]) (.) r[j] on the pattern of a device matrix; g is the
// identity, |v|, v v or 1, the device vectors l (A.rows doubles) and r (A.cols doubles) are optional and each multiplies or
// divides.  Scale(A, params, config) works IN PLACE -- only A's values change --, Scale(A, params, matOut, config) leaves A
// alone.  Every step in double, one rounding to the value type: bit for bit numpy's chain.  No reference counterpart.
// Instantiated for float and double; see speck_scale_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void Scale(dCSR<DataType>& A, const speck_scale_params& params, spECKConfig& config, speck_scale_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_scale_f64(config.handle, &a, &params, nullptr, info)
                                         : speck_scale_f32(config.handle, &a, &params, nullptr, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Scale: ") + speck_status_string(rc));
}

template <typename DataType>
void Scale(const dCSR<DataType>& A, const speck_scale_params& params, dCSR<DataType>& matOut, spECKConfig& config,
           speck_scale_info* info = nullptr)
{
    speck_dcsr a = A.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_scale_f64(config.handle, &a, &params, &c, info)
                                         : speck_scale_f32(config.handle, &a, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Scale: ") + speck_status_string(rc));
}
}  // namespace spECK
