// SortRows.h -- spECK::SortRows: the rows of a device matrix sorted in place by column id (stable), optionally with equal
// columns summed into one entry -- what makes a matrix produced on the device an input of MultiplyspECK.  No reference
// counterpart: its host loader sorts while it converts COO to CSR (source/CSR.cpp:173-212).  Instantiated for float and
// double; see speck_sort_rows_f64 in speck_c_api.h for the contract.
#pragma once
#include <stdexcept>
#include <string>

#include "dCSR.h"

namespace spECK {
template <typename DataType>
void SortRows(dCSR<DataType>& mat, bool sumDuplicates = false)
{
    speck_dcsr m = mat.raw();
    const int flags = sumDuplicates ? SPECK_SORT_SUM_DUPLICATES : SPECK_SORT_KEEP_DUPLICATES;
    const int rc = sizeof(DataType) == 8 ? speck_sort_rows_f64(nullptr, &m, flags, nullptr)
                                         : speck_sort_rows_f32(nullptr, &m, flags, nullptr);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SortRows: ") + speck_status_string(rc));
    mat.adopt(m);  // (same pointers; nnz is smaller when duplicates were summed)
}
}  // namespace spECK
