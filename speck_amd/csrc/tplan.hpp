// tplan.hpp -- speck_tplan: the pattern of a matrix, transposed once (extras.hip makes it with the transpose's sort,
// spmm_t.hip multiplies through it).  One device allocation, four arrays on 256-byte boundaries; after the creation
// nothing writes to it, so any number of calls, streams and configs may read one plan.
#pragma once
#include "host_common.hpp"

struct speck_tplan {
    uint64_t rows, cols, nnz;              // of the matrix the plan was made from
    uint64_t cols_empty, max_col_entries;  // counted once, at the creation
    void* mem;                             // the one allocation
    size_t bytes;
    const speck::u32* t_ro;   // [cols + 1]  the offsets of A^T, from 0
    const speck::u32* t_row;  // [padded]    the row inside A of the e-th entry in column order
    const speck::u32* t_pos;  // [padded]    its position in A, relative to A's first entry
    const speck::u32* ro0;    // [rows + 1]  A's offsets, rebased to 0
};

namespace speck {

// t_row and t_pos reach to the end of the last tile of kPlanTile entries, zeros behind nnz: the thread of a tile kernel
// that holds the last entry loads 16 of each with 16-byte loads like every other
constexpr u32 kPlanTile = 4096;
inline size_t plan_padded(u64 nnz) { return size_t((nnz + kPlanTile - 1) / kPlanTile) * kPlanTile; }

}  // namespace speck
