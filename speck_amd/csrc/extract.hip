// extract.hip -- speck_extract_*: C = A(p, q): the rows of A that a device index list names, in the list's order (repeats
// allowed), every column id sent through a device map that renumbers or drops it; entries in input order, values copied
// bit for bit.  The reference has no counterpart.
//
//   extract_check_kernel   three uniform sections, a thread per item: the rows of A (the family's offset check,
//                          entry_tiles.hpp), the n_rows indices (against rows(A); the length of the gathered row -- 0 where
//                          the index or that row's own two offsets are unsound: clamped, never followed) and the cols(A) map
//                          entries (dropped, or < out_cols).  The gathered entries are summed in 64 bits: a wave reduction,
//                          one atomic per workgroup.  The shared scan (scan.hpp) over the lengths gives the gross offsets G.
//                          FIRST read-back: the verdict and the gross entry count (2^32 or more: refused before any
//                          32-bit offset is used).
//   extract_mark_kernel    one workgroup per tile of 4096 gross entries, four consecutive ones -- one KeepWord word -- per
//                          thread, whatever the row lengths.  The rows of the tile (tile_rows_load): two searches in G, then
//                          the ends and the source offsets of up to 4096 rows in LDS; a tile that more rows touch (thousands
//                          of empty rows between two entries) reads them from global memory instead.  Every id is compared
//                          with cols(A) before it indexes the map.  One 32-bit store of keep bytes per thread; the kept
//                          entries per row counted in LDS, stored for the rows that lie inside the tile, added with one
//                          integer atomic per row and tile for the two that may leave it.  Without a map: the ids are
//                          checked, nothing is written.  The shared scan over the counts gives the new offsets;
//                          offset_stats_kernel (scan.hpp) the empty and the longest row.  SECOND read-back.
//   extract_place_kernel   behind prepare_c and the shared scan over the keep words: the same tiles, the same rows; an
//                          entry's place is the number of kept gross entries in front of it -- no row is looked up for the
//                          destination.  The source position and map[id] are computed again rather than staged by the
//                          marking pass.  Every entry of C is written once, by one thread.
// The host side is the side operations' own (side_call.hpp: the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "compact.hpp"
#include "entry_tiles.hpp"
#include "extract.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kTile = SPECK_EXTRACT_TILE_ENTRIES, kThreads = 1024, kPer = 4;
constexpr u32 kTileRows = 4096;   // rows of a tile whose ends and offsets LDS holds
constexpr u32 kCheckGrid = 2048;  // workgroups of the grid-stride kernels
static_assert(kTile == kThreads * kPer && kTile == kCompactTile, "a thread holds one KeepWord word; a tile is one workgroup of its scan");

struct ExtractStatus {
    u32 invalid;   // offsets of A, a row index, a map value, an id of a gathered row, an input inside A's entries
    u32 max_row;   // the longest row of C
    unsigned long long gross, cols_kept, rows_empty, nnz_out;
};

// what the three passes read.  I: u32, or u64 (an int64_t read as unsigned: a negative value is above every limit)
template <typename I>
struct GatherArgs {
    const u32 *ro, *col;   // A (absolute offsets of a view)
    const I *index, *map;  // either may be null
    const u32* G;          // gross offsets: n + 1
    u32 rows, cols, n, out_cols;
    u64 nnz, gross;
};

template <typename I>
__device__ __forceinline__ bool is_dropped(I m)
{
    if constexpr (sizeof(I) == 8) return (m >> 63) != 0;  // any negative int64_t
    else return m == 0xFFFFFFFFu;
}

// ------------------------------------------------------------------------------------------------ check
// a_data (like g.col): compared with the spans of the index and the map, not read (A's entries start at an offset the device knows)
template <typename I>
__global__ __launch_bounds__(256) void extract_check_kernel(const GatherArgs<I> g, const void* a_data, u32 vsize, u32* __restrict__ gross_len,
                                                            ExtractStatus* st)
{
    SPECK_POISON();
    __shared__ unsigned long long s_gross, s_kept;
    if (threadIdx.x == 0) s_gross = 0, s_kept = 0;
    __syncthreads();
    const u64 first = u64(blockIdx.x) * blockDim.x + threadIdx.x, stride = u64(gridDim.x) * blockDim.x;
    const u32 base = g.rows ? g.ro[0] : 0u;
    bool bad = false;
    // the index and the map against A's entries (every thread, on scalars: an array that lies there is not an index array --
    // it is refused before a word of it is read)
    if (g.nnz) {
        const uintptr_t in[2] = {reinterpret_cast<uintptr_t>(g.index), reinterpret_cast<uintptr_t>(g.map)};
        const u64 in_len[2] = {u64(g.n) * sizeof(I), u64(g.cols) * sizeof(I)};
        const uintptr_t c0 = reinterpret_cast<uintptr_t>(g.col) + u64(base) * 4, d0 = reinterpret_cast<uintptr_t>(a_data) + u64(base) * vsize;
        for (int k = 0; k < 2; ++k) {
            if (!in[k] || !in_len[k]) continue;
            if (g.col && in[k] < c0 + g.nnz * 4 && c0 < in[k] + in_len[k]) bad = true;
            if (a_data && in[k] < d0 + g.nnz * vsize && d0 < in[k] + in_len[k]) bad = true;
        }
        if (bad) {
            if (first == 0) st->invalid = 1;
            return;
        }
    }
    for (u64 r = first; r < g.rows; r += stride) {
        bool empty;
        bad |= !row_offsets_sound<kTile>(g.ro, (u32)r, g.rows, base, g.nnz, 0u, nullptr, &empty);
    }
    u64 gross = 0;
    for (u64 i = first; i < g.n; i += stride) {
        const u64 idx = g.index ? (u64)g.index[i] : i;
        u32 len = 0;
        if (idx < g.rows) {
            const u32 a = g.ro[idx], b = g.ro[idx + 1];
            if (a <= b && a >= base && u64(b) - base <= g.nnz) len = b - a;  // (else: the section above has raised the verdict)
        } else bad = true;
        gross_len[i] = len;
        gross += len;
    }
    u32 kept = 0;
    if (g.map)
        for (u64 j = first; j < g.cols; j += stride) {
            const I m = g.map[j];
            const bool drop = is_dropped(m);
            bad |= !drop && m >= (I)g.out_cols;
            kept += !drop;
        }
    if (bad) st->invalid = 1;
    wave_counter_to_lds(&s_gross, gross);
    wave_counter_to_lds(&s_kept, kept);
    __syncthreads();
    lds_counter_to_status(&st->gross, &s_gross, 0u);
    lds_counter_to_status(&st->cols_kept, &s_kept, 64u);
}

// ------------------------------------------------------------------------------------------------ the rows of a tile
template <typename I>
__device__ __forceinline__ u32 row_source_offset(const GatherArgs<I>& g, u32 r)
{
    // entry e of gathered row r lies at ro[p[r]] + (e - G[r]): the difference, modulo 2^32 (the sum with e is below it)
    return g.ro[g.index ? (u32)g.index[r] : r] - g.G[r];
}

// The rows the gross entries [e0, e1) belong to: r0 .. r0 + nr - 1, the first and the last by a search in G (two threads of
// two waves).  nr <= kTileRows: s_end[k] = G[r0 + k + 1] and s_off[k] = the source offset of row r0 + k.  s_head: four words.
// Ends with a barrier; s_head[2] = G[r0].
template <typename I>
__device__ __forceinline__ void tile_rows_load(const GatherArgs<I>& g, u32 e0, u32 e1, u32* s_end, u32* s_off, u32* s_head, u32* r0_out,
                                               u32* nr_out)
{
    if (threadIdx.x == 0) {
        const u32 r0 = first_end_beyond(g.G + 1, g.n, e0);
        s_head[0] = r0;
        s_head[2] = g.G[r0];
    }
    if (threadIdx.x == 64) s_head[1] = first_end_beyond(g.G + 1, g.n, e1 - 1u);
    __syncthreads();
    const u32 r0 = s_head[0], nr = s_head[1] - r0 + 1u;
    if (nr <= kTileRows)
        for (u32 k = threadIdx.x; k < nr; k += kThreads) {
            s_end[k] = g.G[r0 + k + 1];
            s_off[k] = row_source_offset(g, r0 + k);
        }
    __syncthreads();
    *r0_out = r0, *nr_out = nr;
}

// The thread's cnt <= kPer consecutive gross entries from e on: k[j] = the row (inside the tile) and src[j] = the place in
// A's buffers of entry e + j.  One search for the first, a walk over the ends for the others.
template <typename I, bool kLds>
__device__ __forceinline__ void thread_entries(const GatherArgs<I>& g, const u32* s_end, const u32* s_off, u32 r0, u32 nr, u32 e, u32 cnt,
                                               u32 (&k)[kPer], u32 (&src)[kPer])
{
    const u32* end = kLds ? s_end : g.G + r0 + 1;
    u32 at = cnt ? first_end_beyond(end, nr, e) : nr - 1u;
    u32 off = cnt ? (kLds ? s_off[at] : row_source_offset(g, r0 + at)) : 0u;
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) {
        if (j && j < cnt && end[at] <= e + j) {
            do ++at; while (end[at] <= e + j);  // (ends below nr: the tile's last row ends beyond its last entry)
            off = kLds ? s_off[at] : row_source_offset(g, r0 + at);
        }
        k[j] = at;
        src[j] = off + e + j;
    }
}

// The kept entries (bits 0, 8, 16, 24 of w) of the thread's rows k[0] <= .. <= k[3], added to cnt[k]: a run of one row
// inside the thread is one add, a wave that lies in one row adds once.  Whole waves.
__device__ __forceinline__ void count_kept(u32* cnt, const u32 (&k)[kPer], u32 w)
{
    u32 cur = k[0], c = 0;
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) {
        if (k[j] != cur) {
            if (c) atomicAdd(&cnt[cur], c);
            cur = k[j], c = 0;
        }
        c += (w >> (8u * j)) & 1u;
    }
    const u32 k_first = (u32)__builtin_amdgcn_readfirstlane((int)k[0]), k_last = (u32)__builtin_amdgcn_readlane((int)cur, 63);
    if (k_first == k_last) {
        const u32 total = wave_reduce_add(c);
        if (lane_id() == 0 && total) atomicAdd(&cnt[k_first], total);
    } else if (c) atomicAdd(&cnt[cur], c);
}

// ------------------------------------------------------------------------------------------------ mark
template <typename I>
__global__ __launch_bounds__(kThreads) void extract_mark_kernel(const GatherArgs<I> g, u32* __restrict__ keep32, u32* __restrict__ row_cnt,
                                                                ExtractStatus* st)
{
    SPECK_POISON();
    __shared__ u32 s_end[kTileRows], s_off[kTileRows], s_cnt[kTileRows];
    __shared__ u32 s_head[4];
    const u32 t = threadIdx.x;
    const u64 e0 = u64(blockIdx.x) * kTile, e1 = std::min<u64>(e0 + kTile, g.gross);
#pragma unroll
    for (u32 j = 0; j < kTileRows / kThreads; ++j) s_cnt[t + j * kThreads] = 0;
    u32 r0, nr;
    tile_rows_load(g, (u32)e0, (u32)e1, s_end, s_off, s_head, &r0, &nr);
    const bool lds = nr <= kTileRows;
    const u64 ef = e0 + u64(t) * kPer;
    const u32 cnt = ef < e1 ? (u32)std::min<u64>(kPer, e1 - ef) : 0u;
    u32 k[kPer], src[kPer];
    if (lds) thread_entries<I, true>(g, s_end, s_off, r0, nr, (u32)ef, cnt, k, src);
    else thread_entries<I, false>(g, s_end, s_off, r0, nr, (u32)ef, cnt, k, src);
    u32 id[kPer];
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) id[j] = j < cnt ? g.col[src[j]] : 0u;
    bool bad = false;
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) bad |= id[j] >= g.cols;  // (an idle slot holds 0 -- and cols >= 1 wherever an entry exists, or it is refused)
    if (bad && cnt) st->invalid = 1;
    if (!g.map) return;  // (every entry is kept: nothing to mark, G are the new offsets)
    I m[kPer];
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) m[j] = j < cnt && id[j] < g.cols ? g.map[id[j]] : ~I(0);
    u32 w = 0;
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) w |= (is_dropped(m[j]) ? 0u : 1u) << (8u * j);
    if (cnt) keep32[(e0 >> 2) + t] = w;
    if (!lds) {
        count_kept(row_cnt + r0, k, w);
        return;
    }
    count_kept(s_cnt, k, w);
    __syncthreads();
    for (u32 i = t; i < nr; i += kThreads) {
        const u32 c = s_cnt[i];
        if (!c) continue;  // (the counts were zeroed in front of the pass)
        const bool inside = (i > 0u || s_head[2] >= e0) && (i + 1u < nr || s_end[i] <= e1);
        if (inside) row_cnt[r0 + i] = c;
        else atomicAdd(&row_cnt[r0 + i], c);
    }
}

// ------------------------------------------------------------------------------------------------ place
// keep32 == nullptr (no map): every gross entry goes to its own position
template <typename I, typename T>
__global__ __launch_bounds__(kThreads) void extract_place_kernel(const GatherArgs<I> g, const T* __restrict__ a_val,
                                                                 const u32* __restrict__ keep32, const u32* __restrict__ tile_sums,
                                                                 u32* __restrict__ c_col, T* __restrict__ c_val)
{
    SPECK_POISON();
    __shared__ u32 s_end[kTileRows], s_off[kTileRows];
    __shared__ u32 s_head[4];
    __shared__ u32 s_scan[kThreads / 64 + 1];
    const u32 t = threadIdx.x;
    const u64 e0 = u64(blockIdx.x) * kTile, e1 = std::min<u64>(e0 + kTile, g.gross);
    u32 r0, nr;
    tile_rows_load(g, (u32)e0, (u32)e1, s_end, s_off, s_head, &r0, &nr);
    const u64 ef = e0 + u64(t) * kPer;
    const u32 cnt = ef < e1 ? (u32)std::min<u64>(kPer, e1 - ef) : 0u;
    u32 k[kPer], src[kPer];
    if (nr <= kTileRows) thread_entries<I, true>(g, s_end, s_off, r0, nr, (u32)ef, cnt, k, src);
    else thread_entries<I, false>(g, s_end, s_off, r0, nr, (u32)ef, cnt, k, src);
    u32 w, to;
    if (keep32) {
        w = KeepWord{keep32, g.gross}.word(blockIdx.x * kThreads + t);
        u32 total;
        to = tile_sums[blockIdx.x] + block_exclusive_scan<kThreads>((u32)__popc(w), s_scan, &total);
    } else {
        w = cnt ? 0x01010101u >> (8u * (kPer - cnt)) : 0u;
        to = (u32)ef;
    }
    u32 id[kPer];
    T v[kPer];
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) {
        const bool kept = (w >> (8u * j)) & 1u;
        id[j] = kept ? g.col[src[j]] : 0u;
        v[j] = kept ? a_val[src[j]] : T(0);
    }
    if (g.map) {
#pragma unroll
        for (u32 j = 0; j < kPer; ++j)
            if ((w >> (8u * j)) & 1u) id[j] = (u32)g.map[id[j]];  // (a kept entry: its id and map value passed the marking pass)
    }
#pragma unroll
    for (u32 j = 0; j < kPer; ++j)
        if ((w >> (8u * j)) & 1u) {
            c_col[to] = id[j];
            c_val[to] = v[j];
            ++to;
        }
}

// ------------------------------------------------------------------------------------------------ host
template <typename I, typename T>
int extract_run(ExtractScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_extract_params* p, speck_dcsr* C,
                speck_extract_info* info, COut* out)
{
    const u32 n = (u32)p->n_rows;
    // status | lengths of the gathered rows | G | kept per row | new row offsets | workgroup sums of the scans
    const size_t row_bytes = up256((size_t(n) + 1) * 4), sum_bytes = up256(size_t((n + 1023) / 1024 + 1) * 4);
    int rc = sc->fixed.ensure(256 + 4 * row_bytes + sum_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* fb = static_cast<unsigned char*>(sc->fixed.p);
    static_assert(sizeof(ExtractStatus) <= 256, "status block");
    ExtractStatus* st = reinterpret_cast<ExtractStatus*>(fb);
    u32* gross_len = reinterpret_cast<u32*>(fb + 256);
    u32* G = reinterpret_cast<u32*>(fb + 256 + row_bytes);
    u32* row_cnt = reinterpret_cast<u32*>(fb + 256 + 2 * row_bytes);
    u32* new_ro = reinterpret_cast<u32*>(fb + 256 + 3 * row_bytes);
    u32* block_sums = reinterpret_cast<u32*>(fb + 256 + 4 * row_bytes);

    // ---- the verdict on A's offsets, the indices and the map, and the gathered entries: read before G is used
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(ExtractStatus), s));
    GatherArgs<I> g{A->row_offsets, A->col_ids, static_cast<const I*>(p->d_row_index), static_cast<const I*>(p->d_col_map), G,
                    (u32)A->rows, (u32)A->cols, n, (u32)p->out_cols, A->nnz, 0};
    const u64 items = std::max<u64>(std::max<u64>(A->rows, n), g.map ? A->cols : 0);
    SPECK_LAUNCH(extract_check_kernel<I>, dim3(grid_of((items + 255) / 256, kCheckGrid)), dim3(256), 0, s, g, A->data, (u32)sizeof(T),
                 gross_len, st);
    if (n) launch_exclusive_scan(s, CountArray{gross_len}, n, block_sums, G, nullptr);
    ExtractStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    if (h.gross >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;  // (G wrapped: nothing has read it)
    const u64 gross = h.gross, cols_kept = g.map ? h.cols_kept : A->cols;
    if (n == 0) {
        rc = publish_empty_c(C, p->out_cols, sizeof(T), s, out);
        if (rc == SPECK_OK && info) info->cols_kept = cols_kept;
        return rc;
    }
    g.gross = gross;

    // ---- the ids of the gathered rows, the marks and nnz(C): read before anything of C is allocated or written
    const u32 tiles = (u32)((gross + kTile - 1) / kTile);
    const size_t keep_bytes = up256(std::max<u64>(gross, 1));
    rc = sc->var.ensure(keep_bytes + up256(size_t(std::max(tiles, 1u)) * 4));
    if (rc != SPECK_OK) return rc;
    u32* keep32 = static_cast<u32*>(sc->var.p);
    u32* tile_sums = reinterpret_cast<u32*>(static_cast<unsigned char*>(sc->var.p) + keep_bytes);
    const bool marks = g.map && gross;
    if (marks) HIP_TRY(hipMemsetAsync(row_cnt, 0, (size_t(n) + 1) * 4, s));
    if (gross) SPECK_LAUNCH(extract_mark_kernel<I>, dim3(tiles), dim3(kThreads), 0, s, g, keep32, row_cnt, st);
    if (marks) launch_exclusive_scan(s, CountArray{row_cnt}, n, block_sums, new_ro, &st->nnz_out);
    const u32* c_ro = marks ? new_ro : G;
    SPECK_LAUNCH(offset_stats_kernel, dim3(grid_of((u64(n) + 255) / 256, kCheckGrid)), dim3(256), 0, s, c_ro, n, &st->max_row, &st->rows_empty);
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    const u64 nnz_out = marks ? h.nnz_out : gross;

    // ---- place
    rc = prepare_c(C, n, nnz_out, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    if (nnz_out) {
        if (marks) launch_exclusive_scan(s, KeepWord{keep32, gross}, (u32)((gross + 3) / 4), tile_sums, nullptr, nullptr);
        SPECK_LAUNCH((extract_place_kernel<I, T>), dim3(tiles), dim3(kThreads), 0, s, g, static_cast<const T*>(A->data),
                     marks ? keep32 : nullptr, tile_sums, out->col, static_cast<T*>(out->val));
    }
    rc = finish_rows(s, c_ro, n, p->out_cols, nnz_out, C, out);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->rows_out = n;
        info->rows_empty = h.rows_empty;
        info->gross = gross;
        info->nnz_out = nnz_out;
        info->dropped = gross - nnz_out;
        info->cols_kept = cols_kept;
        info->max_row_entries = h.max_row;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"extract row lengths and offsets", "extract keep bytes", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int extract_impl(speck_config* cfg, const speck_dcsr* A, const speck_extract_params* p, speck_dcsr* C, speck_extract_info* info)
{
    if (!A || !p || !C) return SPECK_ERR_INVALID;
    if (p->index_bytes != 4 && p->index_bytes != 8) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || p->n_rows > (1ull << 27) || p->out_cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (!csr_args_ok(A, true) || (A->nnz && (A->rows == 0 || A->cols == 0))) return SPECK_ERR_INVALID;
    if (!p->d_row_index && p->n_rows != A->rows) return SPECK_ERR_INVALID;
    if (!p->d_col_map && p->out_cols != A->cols) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A)) return SPECK_ERR_INVALID;
    // the index and the map against A's and C's buffers as far as the host knows their place (the entries of a view: the check pass)
    const void* in[2] = {p->d_row_index, p->d_col_map};
    const u64 in_len[2] = {p->n_rows * p->index_bytes, A->cols * p->index_bytes};
    const void* theirs[6] = {A->data, A->col_ids, A->row_offsets, C->data, C->col_ids, C->row_offsets};
    const u64 their_len[6] = {A->nnz * sizeof(T), A->nnz * 4, (A->rows + 1) * 4, C->nnz * sizeof(T), C->nnz * 4, (C->rows + 1) * 4};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 6; ++b)
            if (spans_overlap(in[a], in_len[a], theirs[b], their_len[b])) return SPECK_ERR_INVALID;
    if (info) *info = speck_extract_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, extract_scratch, C, info, kGuardNames, " by the extraction", [&](ExtractScratch* sc, hipStream_t s, COut* out) {
        return p->index_bytes == 8 ? extract_run<u64, T>(sc, s, A, p, C, info, out) : extract_run<u32, T>(sc, s, A, p, C, info, out);
    });
}

}  // namespace

extern "C" {

int speck_extract_f64(speck_config* cfg, const speck_dcsr* A, const speck_extract_params* p, speck_dcsr* C, speck_extract_info* info)
{
    return extract_impl<double>(cfg, A, p, C, info);
}

int speck_extract_f32(speck_config* cfg, const speck_dcsr* A, const speck_extract_params* p, speck_dcsr* C, speck_extract_info* info)
{
    return extract_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
