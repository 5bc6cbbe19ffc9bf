// SpMV.h -- spECK::SpMV: y = alpha A x + beta y on a device matrix; d_x (A.cols doubles, indexed by the column id) and d_y
// (A.rows doubles, indexed by the row inside A) are device arrays of doubles for both value types.  The row sums come
// from the tree of spECK::Reduce(SPECK_REDUCE_SUM): the same bits from run to run, and a row-range view gives the rows of
// the whole matrix bit for bit.  beta == 0 does not read y; a NaN is never hidden.  No reference counterpart.
// Instantiated for float and double; see speck_spmv_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
void SpMV(const dCSR<DataType>& A, const double* d_x, double* d_y, spECKConfig& config, double alpha = 1.0, double beta = 0.0,
          speck_spmv_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmv_f64(config.handle, alpha, &a, d_x, beta, d_y, info)
                                         : speck_spmv_f32(config.handle, alpha, &a, d_x, beta, d_y, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMV: ") + speck_status_string(rc));
}
}  // namespace spECK
