// sort_rows.hpp -- what speck_sort_rows_* (sort_rows.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the row sort: two grow-only allocations of their own (the scratch arena belongs to the multiply: a
// reuse sequence reads what the previous call left in it).  `fixed` is sized from rows(M) before the first kernel
// (status block, class lists, duplicates per row), `var` from what the classifying pass found (long-row ping-pong
// buffers, compaction targets, the copy a refused view is restored from).  Released with the config.
struct SortScratch {
    DeviceBuffer fixed, var;
    u32 reg_max = 256;    // options sort_reg_max / sort_lds_max (clamped to SPECK_SORT_REG_MAX / SPECK_SORT_LDS_MAX)
    u32 lds_max = 4096;
    void release() { fixed.release(), var.release(); }
};

SortScratch* sort_scratch(speck_config* c);
// rows per tile of the classifying pass: the long tile for kSortTileLongRows rows or more of fewer than kSortTileLongAvg entries
constexpr u32 kSortTileRows = 128, kSortTileRowsLong = 512, kSortTileLongRows = 1u << 19, kSortTileLongAvg = 64;

}  // namespace speck
