// Extract.h -- spECK::Extract: matOut = A(p, q): the rows of A that a device index list names, in the list's order (repeats
// allowed), every column id sent through a device map that renumbers or drops it; entries in input order, values bit for
// bit -- an induced subgraph, a permutation P A P^T, a block of a coarse / fine splitting.  No reference counterpart.
// Instantiated for float and double values and both index types; see speck_extract_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "SortRows.h"
#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
// d_row_index: n_rows indices into the rows of A, or nullptr (every row in order: n_rows must be A.rows).  d_col_map: A.cols
// new ids -- int64_t: negative = dropped; uint32_t: 0xFFFFFFFF = dropped --, or nullptr (identity: out_cols must be A.cols).
// canonical: SortRows on the result (a composition here, not in the C call: the extraction itself leaves matOut untouched
// on every error); sumDuplicates (implies canonical) merges equal columns.
template <typename DataType, typename IndexType>
void Extract(const dCSR<DataType>& A, size_t n_rows, const IndexType* d_row_index, size_t out_cols, const IndexType* d_col_map,
             dCSR<DataType>& matOut, spECKConfig& config, speck_extract_info* info = nullptr, bool canonical = false,
             bool sumDuplicates = false)
{
    static_assert(std::is_same<IndexType, uint32_t>::value || std::is_same<IndexType, int64_t>::value, "uint32_t or int64_t ids");
    const speck_extract_params params{n_rows, out_cols, d_row_index, d_col_map, (uint32_t)sizeof(IndexType)};
    speck_dcsr a = A.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_extract_f64(config.handle, &a, &params, &c, info)
                                         : speck_extract_f32(config.handle, &a, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Extract: ") + speck_status_string(rc));
    if (canonical || sumDuplicates) SortRows(matOut, sumDuplicates);
}
}  // namespace spECK
