// select.hpp -- what speck_select_* (select.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the filter: two grow-only allocations of their own (the scratch arena belongs to the multiply: a reuse
// sequence reads what the previous call left in it, and a select between two identical multiplies must not disturb the
// second one).  `fixed` is sized from rows(A) (status block, kept entries per row, the new row offsets, the partial sums
// of their scan), `var` from nnz(A) (one keep byte per entry, the kept entries per tile of the compaction).  Both sizes
// are known before the first kernel.  Released with the config.
struct SelectScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

SelectScratch* select_scratch(speck_config* c);

}  // namespace speck
