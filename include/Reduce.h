// Reduce.h -- spECK::Reduce: per row (d_row_out, a device array of A.rows doubles, may be null) and over all entries
// (h_total, host, may be null) of a device matrix, the sum of v, |v| or v v, or the largest v, smallest v or largest |v|:
// op is one of SPECK_REDUCE_*.  Results are double for both value types; a row without entries is the identity, a NaN is
// never hidden, and a row-range view gives the rows of the whole matrix bit for bit.  No reference counterpart.
// Instantiated for float and double; see speck_reduce_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void Reduce(const dCSR<DataType>& A, int op, double* d_row_out, double* h_total, spECKConfig& config,
            speck_reduce_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_reduce_f64(config.handle, &a, op, d_row_out, h_total, info)
                                         : speck_reduce_f32(config.handle, &a, op, d_row_out, h_total, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Reduce: ") + speck_status_string(rc));
}
}  // namespace spECK
