// topk.hpp -- what speck_topk_* (topk.hip) needs from a config (pipeline.hip owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of the per-row top-k: one grow-only allocation of its own (the scratch arena belongs to the multiply), sized
// from rows(A) before the first kernel: the status block, the six row lists (three regions of `rows` words), the entries a
// row keeps, the new row offsets and the partial sums of their scan.  `var` stays empty: the selection moves nothing and
// has no temporary per entry.  Released with the config.
struct TopKScratch {
    DeviceBuffer fixed, var;
    u32 group_max = SPECK_TOPK_GROUP_MAX;  // options topk_group_max / topk_lds_max (clamped to the defines)
    u32 lds_max = SPECK_TOPK_LDS_MAX;
    void release() { fixed.release(), var.release(); }
};

TopKScratch* topk_scratch(speck_config* c);
// rows per tile of the classifying pass: the long tile for kTopkTileLongRows rows or more of fewer than kTopkTileLongAvg entries
// (the row sort's rule.  Measured on the webbase stand-in's S S, 1 M rows of 52 entries: 396 us with the long tile, 463 us
//  with the short one: DESIGN.md 4.24)
constexpr u32 kTopkTileRows = 128, kTopkTileRowsLong = 512, kTopkTileLongRows = 1u << 19, kTopkTileLongAvg = 64;

}  // namespace speck
