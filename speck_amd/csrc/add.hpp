// add.hpp -- what speck_add_* (add.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the addition: two grow-only allocations of their own, as the filter has them (select.hpp: the scratch
// arena belongs to the multiply, and an add between two identical multiplies must not disturb the second one).  `fixed`
// is sized from the rows (status block, entries of C per row, the row offsets of C, the partial sums of their scan), `var`
// from nnz(A) and nnz(B) (one match byte per entry of either operand, the matches per tile of the write pass, the row in
// which each of those tiles starts, the lower bound of every entry in the other operand's row).  All sizes are known
// before the first kernel.  Released with the config.
struct AddScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

AddScratch* add_scratch(speck_config* c);

}  // namespace speck
