// entry_tiles.hpp -- what the operations that walk a matrix in ENTRY TILES (reduce.hip, scale.hip, spmv.hip, spmm.hip)
// share: the check of one row's offsets in their first pass, which also tells every tile the rows of its first and of its
// last entry.  A tile is the entries [kTile t, kTile (t + 1)) of the buffers, counted from the buffers' start and clipped
// to the matrix; the i-th tile the matrix touches is tile row_offsets[0] / kTile + i.  (What reduce, spmv and spmm do with
// a tile is tile_combine.hpp's; scale.hip has its own pass.)
#pragma once
#include <algorithm>

#include "device_common.hpp"

namespace speck {

// a range of nnz entries touches one tile more than it fills at most: its place is known on the device only
inline u32 entry_tiles_at_most(u64 nnz, u32 tile) { return nnz ? (u32)((nnz + tile - 1) / tile + 1) : 0u; }

#ifdef __HIPCC__
// Row r < rows of a matrix whose first offset is `base`: false where its two offsets descend, leave [base, base + nnz] or,
// for the last row, do not span nnz.  A sound row that holds the first or the last entry of a tile says so in the tile's
// two words, tile_rows[2 i] and [2 i + 1] (null: nobody asks): the pass over the tiles searches nothing.
template <u32 kTile>
__device__ __forceinline__ bool row_offsets_sound(const u32* __restrict__ ro, u32 r, u32 rows, u32 base, u64 nnz, u32 max_tiles,
                                                  u32* __restrict__ tile_rows, bool* empty)
{
    const u32 a = ro[r], b = ro[r + 1];
    bool bad = a > b || a < base || u64(b) - base > nnz;  // (b < base wraps to more than any nnz)
    if (r == rows - 1u) bad |= u64(b) - base != nnz;
    *empty = a == b;
    if (tile_rows && !bad && a < b) {  // (its own offsets are sound: at most as many trips as the matrix has tiles)
        const u64 end = u64(base) + nnz, t_first = base / kTile;
        for (u64 k = a / kTile; k <= (u64(b) - 1) / kTile; ++k) {
            const u64 i = k - t_first, lo = std::max<u64>(k * kTile, base), hi = std::min<u64>((k + 1) * kTile, end);
            if (i >= max_tiles) break;  // (cannot happen: the entries of the row lie inside the matrix)
            if (a <= lo) tile_rows[2 * i] = r;
            if (hi <= b) tile_rows[2 * i + 1] = r;
        }
    }
    return !bad;
}
#endif

}  // namespace speck
