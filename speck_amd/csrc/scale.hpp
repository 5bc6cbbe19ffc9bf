// scale.hpp -- what speck_scale_* (scale.hip) needs from a config (pipeline.hip owns the structure), and what the
// operations that keep A's pattern and write one value per entry, in place or into a new C (scale.hip, sddmm.hip), share
// in front of and behind their own kernels: the status block, the checking pass, C's row offsets.
#pragma once
#include "host_common.hpp"
#ifdef __HIPCC__
#include "entry_tiles.hpp"
#include "launch.hpp"
#endif

namespace speck {

// Temporaries of the scaling: two grow-only allocations of their own, as the reduction has them (the scratch arena
// belongs to the multiply, and a scale between two identical multiplies must not disturb the second one).  `fixed` is the
// status block, `var` the two row words per entry tile (sized from nnz before the first kernel; a call without a row
// vector has no tiles and leaves it alone).  Released with the config.  speck_sddmm_* has a pair of its own.
struct ScaleScratch {
    DeviceBuffer fixed, var;
    void release() { fixed.release(), var.release(); }
};

ScaleScratch* scale_scratch(speck_config* c);
ScaleScratch* sddmm_scratch(speck_config* c);

struct ScaleStatus {
    u32 invalid;  // the offsets, a column id
    u32 base;     // row_offsets[0]
    unsigned long long nonfinite;
};

constexpr u32 kScaleTile = SPECK_SCALE_TILE_ENTRIES, kScaleThreads = 256;
constexpr u32 kColBlocks = 1024, kColUnroll = 4;

#ifdef __HIPCC__
// Two kinds of workgroups in one launch.  A thread per row: the offsets ascend, stay inside [row_offsets[0],
// row_offsets[0] + nnz] and the last one spans nnz (entry_tiles.hpp); with tile_rows a row also tells every entry tile
// the rows of its first and last entry.  Behind them (grid beyond row_blocks): a stream over the ids, each < cols.
static __global__ __launch_bounds__(kScaleThreads) void scale_check_kernel(const u32* __restrict__ ro, const u32* __restrict__ col,
                                                                            u32 rows, u32 cols, u64 nnz, u32 row_blocks,
                                                                            u32 max_tiles, u32* __restrict__ tile_rows, ScaleStatus* st)
{
    SPECK_POISON();
    constexpr u32 kThreads = kScaleThreads;
    const u32 base = ro[0];
    if (blockIdx.x < row_blocks) {
        const u32 r = blockIdx.x * kThreads + threadIdx.x;
        if (r == 0) st->base = base;
        bool empty;
        if (r < rows && !row_offsets_sound<kScaleTile>(ro, r, rows, base, nnz, max_tiles, tile_rows, &empty)) st->invalid = 1;
    } else {
        // the ids of the entries [base, base + nnz), a batch of loads per trip (compared, never followed)
        const u64 stride = u64(gridDim.x - row_blocks) * kThreads * kColUnroll;
        bool bad = false;
        for (u64 b = u64(blockIdx.x - row_blocks) * kThreads * kColUnroll; b < nnz; b += stride) {
            u32 c[kColUnroll];
#pragma unroll
            for (u32 k = 0; k < kColUnroll; ++k) {
                const u64 i = b + k * kThreads + threadIdx.x;
                c[k] = i < nnz ? col[u64(base) + i] : 0u;
            }
#pragma unroll
            for (u32 k = 0; k < kColUnroll; ++k) bad |= b + k * kThreads + threadIdx.x < nnz && c[k] >= cols;
        }
        if (bad) st->invalid = 1;
    }
}

// a new C only: its row offsets, rebased to 0
static __global__ __launch_bounds__(kScaleThreads) void scale_offsets_kernel(const u32* __restrict__ ro, u32 rows, u32* __restrict__ c_ro,
                                                                              const ScaleStatus* st)
{
    SPECK_POISON();
    if (st->invalid) return;
    const u32 r = blockIdx.x * kScaleThreads + threadIdx.x;
    if (r <= rows) c_ro[r] = ro[r] - st->base;
}

// the checking pass of A (rows >= 1) queued on s; check_ids: col_ids is read at all
static inline void launch_scale_check(hipStream_t s, const speck_dcsr* A, bool check_ids, u32 max_tiles, u32* tile_rows, ScaleStatus* st)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz = A->nnz;
    const u32 row_blocks = (rows + kScaleThreads - 1) / kScaleThreads;
    const u32 col_blocks = check_ids && nnz ? grid_of((nnz + kScaleThreads * kColUnroll - 1) / (kScaleThreads * kColUnroll), kColBlocks) : 0u;
    SPECK_LAUNCH(scale_check_kernel, dim3(row_blocks + col_blocks), dim3(kScaleThreads), 0, s, A->row_offsets, A->col_ids, rows,
                 (u32)A->cols, nnz, row_blocks, max_tiles, tile_rows, st);
}

static inline void launch_scale_offsets(hipStream_t s, const speck_dcsr* A, u32* c_ro, const ScaleStatus* st)
{
    SPECK_LAUNCH(scale_offsets_kernel, dim3((u32)A->rows / kScaleThreads + 1), dim3(kScaleThreads), 0, s, A->row_offsets, (u32)A->rows,
                 c_ro, st);
}
#endif

}  // namespace speck
