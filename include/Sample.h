// Sample.h -- spECK::Sample: row i of matOut = at most k entries of row rows[i] of A, chosen uniformly at random -- the
// fan-out neighbour sampling in front of a mini-batch.  An entry's random key is a pure function of (seed, global row, place
// in the row): the same sample from run to run, whatever the values, the ids or the value type.  No reference counterpart.
// Instantiated for float and double; see speck_sample_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
// mode: SPECK_SAMPLE_WITHOUT_REPLACEMENT or SPECK_SAMPLE_WITH_REPLACEMENT.  d_row_index: n_rows DEVICE indices of
// index_bytes (4: uint32_t, 8: int64_t) each, or nullptr for every row of A in order (n_rows is then ignored).  row_base: the
// global index of A's first row where A is a row-range view.  On an error matOut is what it was.
template <typename DataType>
void Sample(const dCSR<DataType>& A, uint64_t k, uint64_t seed, int mode, dCSR<DataType>& matOut, spECKConfig& config,
            const void* d_row_index = nullptr, uint64_t n_rows = 0, uint32_t index_bytes = 8, uint64_t row_base = 0,
            speck_sample_info* info = nullptr)
{
    speck_dcsr a = A.raw(), c = matOut.raw();
    const speck_sample_params params{k, seed, row_base, d_row_index ? n_rows : a.rows, d_row_index, index_bytes, (uint32_t)mode};
    const int rc = sizeof(DataType) == 8 ? speck_sample_f64(config.handle, &a, &params, &c, info)
                                         : speck_sample_f32(config.handle, &a, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::Sample: ") + speck_status_string(rc));
}
}  // namespace spECK
