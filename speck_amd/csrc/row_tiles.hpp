// row_tiles.hpp -- the device side of what the side operations (sort_rows.hip, masked.hip, select.hip, add.hip) share beside
// the scan (scan.hpp) and the compaction (compact.hpp).  Their first pass walks the rows in TILES: a workgroup takes a
// tile's row offsets into LDS, checks them, and only then walks the tile's entries a thread per entry.  Here: the offset
// check, the check of a mask / pattern, the search in a row, the per-row count, a counter's way to the status block, and
// the masked product's walk.  Every helper is inlined: a kernel keeps its barriers, its LDS and its launch shape.
#pragma once
#include "device_common.hpp"

namespace speck {

// "No offset is used as an address before it was checked" rests on these two and the barriers around them.  The tile of
// `nr` rows from row r0 on, kThreads threads, one operand or several:
//     s_bad = 0;  barrier;  tile_offsets_load once per operand;  barrier;  if (tile_offsets_descend(..) || ..) s_bad = 1;
//     barrier;  if (s_bad) { thread 0: st->invalid = 1;  return; }
// Behind it s_ro[0 .. nr] are monotone and inside [base, base + nnz]; base = row_offsets[0] (a view's offsets are absolute).
template <u32 kThreads>
__device__ __forceinline__ void tile_offsets_load(const u32* __restrict__ ro, u32 r0, u32 nr, u32 base, u64 nnz, u32* s_ro, u32* s_bad)
{
    for (u32 i = threadIdx.x; i <= nr; i += kThreads) {
        const u32 o = ro[r0 + i];
        s_ro[i] = o;
        if (o < base || u64(o - base) > nnz) *s_bad = 1;
    }
}

// "my row ends before it starts" (needs at least nr threads)
__device__ __forceinline__ bool tile_offsets_descend(const u32* s_ro, u32 nr)
{
    return threadIdx.x < nr && s_ro[threadIdx.x] > s_ro[threadIdx.x + 1];
}

// The tile's entries of a mask / pattern, a thread per entry: false where one this thread saw is >= cols or not above its
// predecessor although it does not start a row.  (s_ro: the tile's checked offsets.)
template <u32 kThreads>
__device__ __forceinline__ bool rows_ascending_below(const u32* __restrict__ col, const u32* s_ro, u32 nr, u32 cols)
{
    bool unsorted = false;
    const u64 lo = s_ro[0], hi = s_ro[nr];
#pragma unroll 4
    for (u64 i = lo + threadIdx.x; i < hi; i += kThreads) {
        const u32 c = col[i];
        unsorted |= c >= cols;
        if (i > lo && col[i - 1] >= c) unsorted |= i > s_ro[first_end_beyond(s_ro + 1, nr, i)];  // (not the first entry of its row)
    }
    return !unsorted;
}

// The first entry in [lo, hi) of col whose column is >= c (hi: none).  What col holds there is compared, never followed.
__device__ __forceinline__ u32 lower_bound_in_row(const u32* __restrict__ col, u32 lo, u32 hi, u32 c)
{
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (col[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// An entry of row r counts where `flag`.  Whole waves, consecutive entries: one LDS atomic where they lie in one row.
__device__ __forceinline__ void count_entry_in_row(u32* s_cnt, u32 r, bool flag)
{
    const u32 r_first = (u32)__builtin_amdgcn_readfirstlane((int)r), r_last = (u32)__builtin_amdgcn_readlane((int)r, 63);
    if (r_first == r_last) {
        const u64 m = __ballot(flag);
        if (lane_id() == 0 && m) atomicAdd(&s_cnt[r_first], (u32)__popcll(m));
    } else if (flag) atomicAdd(&s_cnt[r], 1u);
}

// wave sum -> one LDS atomic per wave -> ONE global atomic per workgroup (atomics of every wave on the same few words of
// global memory cost ~8 ns each, one after the other: masked.hip).  *s_word: zero, and a barrier, before the first call.
template <typename V>
__device__ __forceinline__ void wave_counter_to_lds(unsigned long long* s_word, V value)
{
    value = wave_reduce_add(value);
    if (lane_id() == 0 && value) atomicAdd(s_word, (unsigned long long)value);
}

// behind the barrier that completes *s_word: thread `issuer` hands it on (several counters: threads of different waves)
template <typename W>
__device__ __forceinline__ void lds_counter_to_status(W* status_word, const W* s_word, u32 issuer)
{
    if (threadIdx.x == issuer && *s_word) atomicAdd(status_word, *s_word);
}

// the two with their barrier, for a kernel with one counter
template <typename V>
__device__ __forceinline__ void block_counter_to(unsigned long long* status_word, V value, unsigned long long* s_word)
{
    wave_counter_to_lds(s_word, value);
    __syncthreads();
    lds_counter_to_status(status_word, s_word, 0u);
}

// (masked.hip, "the product walk": end, off)  The kStride lanes of a group (a sub-wave, a workgroup) stride over the batch's
// products from `first` (a lane's place in its group) on, four loads of B's columns in flight per lane: a walk is a chain
// of such loads otherwise.  apply(i, j, c): entry i of the batch times entry j of B, whose column is c (kNoColumn: none).
constexpr u32 kNoColumn = 0xFFFFFFFFu;  // above every column id (< 2^27)

template <u32 kStride, typename Apply>
__device__ __forceinline__ void walk_products(u32 first, const u32* end, const u32* off, u32 nb, u32 total, const u32* b_col,
                                              Apply&& apply)
{
    for (u32 p = first; p < total; p += 4u * kStride) {
        u32 i[4], j[4], c[4];
#pragma unroll
        for (u32 u = 0; u < 4; ++u) {
            const u32 q = p + u * kStride;
            i[u] = q < total ? first_end_beyond(end, nb, q) : 0u;
            j[u] = off[i[u]] + q;
            c[u] = q < total ? b_col[j[u]] : kNoColumn;
        }
#pragma unroll
        for (u32 u = 0; u < 4; ++u) apply(i[u], j[u], c[u]);
    }
}

}  // namespace speck
