// FromCOO.h -- spECK::FromCOO: device COO triplets (row ids, column ids, values; the ids uint32_t or int64_t, in any order)
// grouped by row into a device matrix, stable and with every id checked before it is followed; spECK::ToCOO: the rows of
// a device matrix expanded into one row index per entry.  The reference converts on the host only (convert(CSR&, const
// COO&), source/CSR.cpp:173-212).  Instantiated for float and double values and both index types; see speck_from_coo_f64
// and speck_to_coo in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "SortRows.h"
#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
// d_val == nullptr: every value is 1.0.  canonical: SortRows on the result (a composition here, not in the C call: the
// conversion itself leaves `out` untouched on every error); sumDuplicates (implies canonical) merges equal columns.
template <typename DataType, typename IndexType>
void FromCOO(dCSR<DataType>& out, size_t rows, size_t cols, size_t nnz, const IndexType* d_row, const IndexType* d_col,
             const DataType* d_val, spECKConfig& config, bool canonical = false, bool sumDuplicates = false,
             speck_from_coo_info* info = nullptr)
{
    static_assert(std::is_same<IndexType, uint32_t>::value || std::is_same<IndexType, int64_t>::value, "uint32_t or int64_t ids");
    const speck_dcoo coo{rows, cols, nnz, d_val, d_row, d_col, (uint32_t)sizeof(IndexType)};
    speck_dcsr c = out.raw();
    const int rc = sizeof(DataType) == 8 ? speck_from_coo_f64(config.handle, &coo, &c, info)
                                         : speck_from_coo_f32(config.handle, &coo, &c, info);
    out.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::FromCOO: ") + speck_status_string(rc));
    if (canonical || sumDuplicates) SortRows(out, sumDuplicates);
}

// d_row_out (and d_col_out, unless nullptr): A.nnz indices each; row_base: the global index of A's first row
template <typename IndexType, typename DataType>
void ToCOO(const dCSR<DataType>& A, IndexType* d_row_out, IndexType* d_col_out, spECKConfig& config, uint64_t row_base = 0)
{
    static_assert(std::is_same<IndexType, uint32_t>::value || std::is_same<IndexType, int64_t>::value, "uint32_t or int64_t ids");
    const speck_dcsr a = A.raw();
    const int rc = speck_to_coo(config.handle, &a, (uint32_t)sizeof(IndexType), row_base, d_row_out, d_col_out);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::ToCOO: ") + speck_status_string(rc));
}
}  // namespace spECK
