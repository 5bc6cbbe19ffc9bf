// spmv.hpp -- what speck_spmv_* (spmv.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the matrix-vector product: three grow-only allocations of their own, as the reduction has two (the
// scratch arena belongs to the multiply, and a spmv between two identical multiplies must not disturb the second one).
// `fixed` is the status block, `var` one record and two row words per entry tile (sized from nnz before the first
// kernel), `sums` the row sums s_i that wait for the verdict on the column ids (rows doubles).  Released with the config.
struct SpmvScratch {
    DeviceBuffer fixed, var, sums;
    void release() { fixed.release(), var.release(), sums.release(); }
};

SpmvScratch* spmv_scratch(speck_config* c);

}  // namespace speck
