// scale.hpp -- what speck_scale_* (scale.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the scaling: two grow-only allocations of their own, as the reduction has them (the scratch arena
// belongs to the multiply, and a scale between two identical multiplies must not disturb the second one).  `fixed` is the
// status block, `var` the two row words per entry tile (sized from nnz before the first kernel; a call without a row
// vector has no tiles and leaves it alone).  Released with the config.
struct ScaleScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

ScaleScratch* scale_scratch(speck_config* c);

}  // namespace speck
