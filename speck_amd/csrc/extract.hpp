// extract.hpp -- what speck_extract_* (extract.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the extraction: two grow-only allocations of their own, as the filter has them (the scratch arena
// belongs to the multiply).  `fixed`, sized from n_rows before the first kernel: the status block, the gathered rows'
// lengths, their gross offsets G, the kept entries per row, the new row offsets and the partial sums of their scans.
// `var`, sized from the gross entry count behind the first read-back (nothing of C exists yet): one keep byte per
// gathered entry and the kept entries per tile of the placing pass.  Released with the config.
struct ExtractScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

ExtractScratch* extract_scratch(speck_config* c);

}  // namespace speck
