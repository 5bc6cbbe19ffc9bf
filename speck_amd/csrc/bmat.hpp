// bmat.hpp -- what speck_bmat_* (bmat.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the assembly: two grow-only allocations of their own, as the extraction has them (the scratch arena
// belongs to the multiply).  `fixed`, sized from the grid and rows(C) before the first kernel: the status block, the
// uploaded tables (the blocks and the groups of block rows), the staged row offsets and the partial sums of the scan.
// `var`, sized from the pieces: a length per piece and their scan G, 8 bytes per piece.  Released with the config.
struct BmatScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

BmatScratch* bmat_scratch(speck_config* c);

}  // namespace speck
