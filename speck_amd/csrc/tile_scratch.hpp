// tile_scratch.hpp -- what speck_reduce_*, speck_spmv_*, speck_spmm_*, speck_softmax_*, speck_spmm_t_*, speck_spmv_sr_* and
// speck_spmm_sr_* (reduce.hip, spmv.hip, spmm.hip, softmax.hip, spmm_t.hip, semiring.hip) need from a config (pipeline.hip
// owns the structure).
#pragma once
#include "host_common.hpp"

namespace speck {

// Temporaries of a call over entry tiles (tile_call.hpp carves them): grow-only allocations of their own, as the filter
// and the addition have them (the scratch arena belongs to the multiply, and a reduce between two identical multiplies
// must not disturb the second one).  `fixed` is the status block; `var` the records of every entry tile -- one per tile,
// k per tile for k right-hand sides -- and two row words per tile, sized from nnz before the first kernel; `sums` the row
// sums of the two products, which wait for the verdict on the column ids (rows, rows k doubles; the reduction leaves it
// empty; the softmax keeps there the m and s of the rows that leave a tile where the caller takes no vector, 2 rows
// doubles).  The config holds one per operation: a spmv after a spmm of many columns keeps its small buffers.  Released
// with the config.
struct TileScratch {
    DeviceBuffer fixed, var, sums;
    void release() { fixed.release(), var.release(), sums.release(); }
};

TileScratch* reduce_scratch(speck_config* c);
TileScratch* spmv_scratch(speck_config* c);
TileScratch* spmm_scratch(speck_config* c);
TileScratch* softmax_scratch(speck_config* c);
TileScratch* spmm_t_scratch(speck_config* c);
// (semiring.hip: neither spmv's nor spmm's -- a wide spmm_sr does not grow the buffers of a spmv)
TileScratch* spmv_sr_scratch(speck_config* c);
TileScratch* spmm_sr_scratch(speck_config* c);

}  // namespace speck
