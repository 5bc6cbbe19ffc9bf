// reduce.hpp -- what speck_reduce_* (reduce.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the reduction: two grow-only allocations of their own, as the filter and the addition have them (the
// scratch arena belongs to the multiply, and a reduce between two identical multiplies must not disturb the second one).
// `fixed` is the status block, `var` one record per entry tile (sized from nnz before the first kernel).  Released with
// the config.
struct ReduceScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

ReduceScratch* reduce_scratch(speck_config* c);

}  // namespace speck
