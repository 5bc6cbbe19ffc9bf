// masked.hpp -- what speck_multiply_masked_* (masked.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the masked product: two grow-only allocations of their own (the scratch arena belongs to the multiply: a
// reuse sequence reads what the previous call left in it, and a masked call between two identical multiplies must not
// disturb the second one).  `fixed` is sized from rows(A) (status block, class lists, hits per row, the new row offsets,
// the partial sums of their scan), `var` from nnz(M) (one double accumulator and one hit byte per mask entry).  Both sizes
// are known before the first kernel.  Released with the config.
struct MaskedScratch {
    DeviceBuffer fixed, var;
    // the class kernels work on disjoint rows: they run side by side, on three streams of the call's own between a fork
    // and a join on the config's stream (created with the first call that has two classes to run)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[3] = {nullptr, nullptr, nullptr};
    u32 group_max = 256;  // options mask_group_max / mask_lds_max (clamped to SPECK_MASK_GROUP_MAX / SPECK_MASK_LDS_MAX)
    u32 lds_max = 4096;
    void release();
};

MaskedScratch* masked_scratch(speck_config* c);
// rows per tile of the classifying pass: the first where a row of A and of M together hold kMaskLongRowAvg entries or more
constexpr u32 kMaskTileRowsLong = 256, kMaskTileRowsShort = 1024, kMaskLongRowAvg = 32;

}  // namespace speck
