// spmm.hpp -- what speck_spmm_* (spmm.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the product with several right-hand sides: three grow-only allocations of their own (not the multiply's
// arena, and not SpmvScratch: a spmv after a spmm of many columns keeps its small buffers).  `fixed` is the status block,
// `var` k records per entry tile and two row words per tile (sized from nnz and k before the first kernel), `sums` the row
// sums s(i,c) that wait for the verdict on the column ids (rows k doubles).  Released with the config.
struct SpmmScratch {
    DeviceBuffer fixed, var, sums;
    void release() { fixed.release(), var.release(), sums.release(); }
};

SpmmScratch* spmm_scratch(speck_config* c);

}  // namespace speck
