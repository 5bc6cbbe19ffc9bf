// sample.hpp -- what speck_sample_* (sample.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the neighbour sampling: one grow-only allocation of its own (the scratch arena belongs to the multiply),
// sized from n_rows before the first kernel: the status block, the six row lists (three regions of n_rows words), and per
// output row its source row, its gathered length, its gross offset, its output length, its new offset; the partial sums of
// the scans.  `var` stays empty: keys are recomputed, never stored -- there is no temporary per entry.  Released with the
// config.
struct SampleScratch {
    DeviceBuffer fixed, var;
    u32 group_max = SPECK_SAMPLE_GROUP_MAX;  // options sample_group_max / sample_lds_max (clamped to the defines)
    u32 lds_max = SPECK_SAMPLE_LDS_MAX;
    void release() { fixed.release(), var.release(); }
};

SampleScratch* sample_scratch(speck_config* c);

}  // namespace speck
