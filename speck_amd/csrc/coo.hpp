// coo.hpp -- what speck_from_coo_* and speck_to_coo (coo.hip) need from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the two conversions: grow-only allocations of their own, as the filter has them (the scratch arena
// belongs to the multiply).  `fixed` is the status block; `var`, sized from nnz before the first kernel, holds the row
// keys the check pass writes and -- carved whether the sort runs or not, so that a call never grows it behind its
// verdict -- the second key buffer, the two position buffers and the histogram of the radix sort (radix_pairs.hpp).
// speck_to_coo uses `fixed` alone.  Released with the config.
struct CooScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

CooScratch* coo_scratch(speck_config* c);

}  // namespace speck
