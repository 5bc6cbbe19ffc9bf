// TopK.h -- spECK::TopK: matOut = the k best entries of every row of A -- by value, by -value or by magnitude --, in input
// order, ids and values bit for bit: the pruning of an MCL step, a kNN graph from scores, top-k attention.  A NaN ranks
// above every number; of equal keys the entry that comes first in its row wins.  No reference counterpart.
// Instantiated for float and double; see speck_topk_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
// mode: SPECK_TOPK_LARGEST, SPECK_TOPK_SMALLEST or SPECK_TOPK_LARGEST_ABS.  On an error matOut is what it was.
template <typename DataType>
void TopK(const dCSR<DataType>& A, uint64_t k, int mode, dCSR<DataType>& matOut, spECKConfig& config, speck_topk_info* info = nullptr)
{
    const speck_topk_params params{k, (uint32_t)mode, 0u};
    speck_dcsr a = A.raw(), c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_topk_f64(config.handle, &a, &params, &c, info)
                                         : speck_topk_f32(config.handle, &a, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::TopK: ") + speck_status_string(rc));
}
}  // namespace spECK
