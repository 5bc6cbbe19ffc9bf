// sample.hip -- speck_sample_*: row i of C = at most k entries of row p[i] of A, chosen uniformly at random, without
// replacement (in input order) or with it (in draw order), copied bit for bit.  The reference has no counterpart.
// The random key of an entry is a pure function of (seed, global row, place in the row) -- two rounds of the SplitMix64
// finaliser, speck_c_api.h -- so a key is never stored or loaded: it is computed where it is needed.
//
//   sample_check_kernel    uniform sections, a thread per item, the shape of extract_check_kernel: the rows of A (the
//                          family's offset check, entry_tiles.hpp) and the n_rows indices (against rows(A); the length of
//                          the gathered row -- 0 where the index or that row's own two offsets are unsound: clamped, never
//                          followed).  Per output row: its source row, its gathered length, its output length -- min(len, k)
//                          or (len ? k : 0).  The 64-bit sums of both lengths.  Mode 0: the rows longer than k go to one of
//                          six lists by length (wave-aggregated integer cursors).  The shared scan (scan.hpp) gives C's
//                          offsets -- they depend on the lengths alone: no marking pass, no keep byte -- and the gross
//                          offsets G.
//   sample_ids_kernel      tiles of 4096 gross entries over the gathered rows, whatever the row lengths (a hub named 1000
//                          times is just many tiles): every id compared with cols(A).  extract's MARK pass without a map.
//                          Its grid strides and it reads the gross count on the device: there is no read-back in front of it.
//                          The ONE read-back in front of C: the verdict, nnz(C), the list lengths.
//   sample_copy_kernel     mode 0, the rows of at most k entries: topk_copy_kernel over gathered rows.
//   sample_group_kernel<L> mode 0, cut rows of <= 4 L entries, L = 8 / 16 / 32 / 64 lanes per row: the row's keys computed
//                          into LDS; every lane counts, for its (up to) four entries, the entries that beat them.
//   sample_row_kernel      mode 0, one workgroup per longer cut row: the radix select and the ordered walk of topk_row_kernel.
//                          kLds: 256 threads, the keys computed ONCE into LDS (<= SPECK_SAMPLE_LDS_MAX).  Otherwise 1024
//                          threads and the keys RECOMPUTED in every pass: the select reads no memory at all.
//   sample_draw_kernel     mode 1: one stream over the output entries, a tile of 4096 per workgroup; the row by a search in
//                          C's offsets, the source place (key * len) >> 64.  Every entry is independent.
// The selection works on ~key: "a smaller (key, t) wins" becomes topk's rule -- a larger key beats, of equal keys the entry
// in front.  The bodies are twins of topk.hip's, not shared with it: there a key is a function of a loaded value of T (32
// or 64 bits wide), the row is a row of A, and the kernels count NaNs and ties on the way; here a key is always 64 bits,
// computed from the place, the row comes through an index list, and nothing else is counted.  A shared body would have
// to be parameterised in all four and topk's kernels rebuilt around it.
// Keys, counts and offsets are integers everywhere: no floating-point atomic and no floating-point arithmetic at all.
// The host side is the side operations' own (side_call.hpp: scratch, status, the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "compact.hpp"
#include "entry_tiles.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "sample.hpp"
#include "scan.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kGroupMax = SPECK_SAMPLE_GROUP_MAX, kLdsMax = SPECK_SAMPLE_LDS_MAX;
constexpr u32 kTile = SPECK_SAMPLE_TILE_ENTRIES, kTileThreads = 1024;
constexpr u32 kPer = 4;  // entries a lane of a group holds; entries a thread of the row and tile kernels keeps in flight
static_assert(kGroupMax == 64 * kPer, "the widest group is a wave");
static_assert(kTile == kTileThreads * kPer, "a tile is one trip of its workgroup");
enum { LIST_G8 = 0, LIST_G16, LIST_G32, LIST_G64, LIST_LDS, LIST_LONG, SAMPLE_LISTS };
constexpr u32 kCheckGrid = 2048, kIdsGrid = 1024;                                           // workgroups of the grid-stride kernels
constexpr u32 kGroupGrid = 2048, kLdsGrid = 2048, kLongGrid = 1024, kCopyTileRows = 256;  // workgroups of a launch at most
constexpr u32 kTileRows = 4096;  // rows of a tile whose ends LDS holds

constexpr u64 kSampleEntriesMax = (1ull << 32) - 1024;  // of A, and of the gathered rows: SPECK_ERR_NNZ_OVERFLOW beyond

struct SampleStatus {
    u32 invalid;             // offsets of A, a row index, an id of a gathered row, the index inside A's entries
    u32 max_row;             // the longest row of C
    u32 cnt[SAMPLE_LISTS];   // list lengths
    unsigned long long gross, nnz_out, rows_empty, rows_cut;
};

// (the six lists share three regions of n_rows words: two_sided_at, device_common.hpp)

// what the kernels behind the check read: per output row i its source row, its gathered length, its gross offset
struct Gathered {
    const u32 *ro, *col;                  // A (absolute offsets of a view)
    const u32 *srow, *glen, *G, *new_ro;  // n, n, n + 1, n + 1
    u32 n, cols, k;
    u64 seed, row_base;
};

// ------------------------------------------------------------------------------------------------ keys
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ u64 mix64(u64 z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ u64 row_key_of(const Gathered& g, u32 i) { return mix64(g.seed + kGolden * (g.row_base + g.srow[i] + 1ull)); }
__device__ __forceinline__ u64 key_at(u64 row_key, u64 t) { return mix64(row_key + kGolden * (t + 1ull)); }
// the selection's key: a larger one beats
__device__ __forceinline__ u64 rank_key_at(u64 row_key, u64 t) { return ~key_at(row_key, t); }

// ------------------------------------------------------------------------------------------------ check
// a_data (like col): compared with the span of the index, not read (A's entries start at an offset the device knows)
template <typename I>
__global__ __launch_bounds__(256) void sample_check_kernel(const u32* __restrict__ ro, const u32* col, const void* a_data, u32 vsize,
                                                           const I* index, u32 rows, u32 n, u64 nnz, u32 k, u64 k_draw, u32 mode,
                                                           u32 group_max, u32 lds_max, u32* __restrict__ srow, u32* __restrict__ glen,
                                                           u32* __restrict__ row_cnt, u32* __restrict__ lists, SampleStatus* st)
{
    SPECK_POISON();
    __shared__ unsigned long long s_gross, s_out, s_empty, s_cut;
    if (threadIdx.x == 0) s_gross = 0, s_out = 0, s_empty = 0, s_cut = 0;
    __syncthreads();
    const u64 first = u64(blockIdx.x) * blockDim.x + threadIdx.x, stride = u64(gridDim.x) * blockDim.x;
    const u32 base = rows ? ro[0] : 0u;
    bool bad = false;
    // the index against A's entries (every thread, on scalars: an array that lies there is not an index array -- it is
    // refused before a word of it is read)
    if (nnz && index && n) {
        const uintptr_t in = reinterpret_cast<uintptr_t>(index);
        const u64 in_len = u64(n) * sizeof(I);
        const uintptr_t c0 = reinterpret_cast<uintptr_t>(col) + u64(base) * 4, d0 = reinterpret_cast<uintptr_t>(a_data) + u64(base) * vsize;
        if (col && in < c0 + nnz * 4 && c0 < in + in_len) bad = true;
        if (a_data && in < d0 + nnz * vsize && d0 < in + in_len) bad = true;
        if (bad) {
            if (first == 0) st->invalid = 1;
            return;
        }
    }
    for (u64 r = first; r < rows; r += stride) {
        bool empty;
        bad |= !row_offsets_sound<kTile>(ro, (u32)r, rows, base, nnz, 0u, nullptr, &empty);
    }
    u64 gross = 0, total_out = 0;
    u32 empties = 0, cuts = 0;
    const u32 lane = lane_id();
    for (u64 i0 = u64(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) {  // (whole waves: the lists are placed by ballot)
        const u64 i = i0 + threadIdx.x;
        const bool on = i < n;
        int cls = -1;  // no row, or a row the copy or the draw takes
        u32 kept = 0;
        if (on) {
            const u64 idx = index ? (u64)index[i] : i;
            u32 len = 0, src = 0;
            if (idx < rows) {
                src = (u32)idx;
                const u32 a = ro[idx], b = ro[idx + 1];
                if (a <= b && a >= base && u64(b) - base <= nnz) len = b - a;  // (else: the section above has raised the verdict)
            } else bad = true;
            const u64 out = mode == SPECK_SAMPLE_WITH_REPLACEMENT ? (len ? k_draw : 0ull) : (u64)min(len, k);
            kept = (u32)out;  // (2^32 or more in one row: the sum refuses the call before anybody reads this)
            srow[i] = src;
            glen[i] = len;
            row_cnt[i] = kept;
            gross += len;
            total_out += out;
            empties += out == 0;
            cuts += len > k;
            if (mode == SPECK_SAMPLE_WITHOUT_REPLACEMENT && len > k) {
                if (len <= group_max && len <= kGroupMax)
                    cls = len <= kGroupMax / 8 ? LIST_G8 : len <= kGroupMax / 4 ? LIST_G16 : len <= kGroupMax / 2 ? LIST_G32 : LIST_G64;
                else cls = (len <= lds_max && len <= kLdsMax) ? LIST_LDS : LIST_LONG;
            }
        }
        const u32 longest = wave_reduce_max(kept);
        if (lane == 0 && longest) atomicMax(&st->max_row, longest);
#pragma unroll
        for (int c = 0; c < SAMPLE_LISTS; ++c) {
            const u64 m = __ballot(cls == c);
            if (m == 0) continue;
            const u32 leader = (u32)__ffsll((long long)m) - 1u;
            u32 at = 0;
            if (lane == leader) at = atomicAdd(&st->cnt[c], (u32)__popcll(m));
            at = (u32)__shfl((int)at, (int)leader);
            if (cls == c) *two_sided_at(lists, n, c, at + (u32)__popcll(m & lanemask_lt())) = (u32)i;
        }
    }
    if (bad) st->invalid = 1;
    wave_counter_to_lds(&s_gross, gross);
    wave_counter_to_lds(&s_out, total_out);
    wave_counter_to_lds(&s_empty, empties);
    wave_counter_to_lds(&s_cut, cuts);
    __syncthreads();
    lds_counter_to_status(&st->gross, &s_gross, 0u);
    lds_counter_to_status(&st->nnz_out, &s_out, 64u);
    lds_counter_to_status(&st->rows_empty, &s_empty, 128u);
    lds_counter_to_status(&st->rows_cut, &s_cut, 192u);
}

// ------------------------------------------------------------------------------------------------ the rows of a tile
// The rows the entries [e0, e1) of the offsets off[0 .. n] belong to: r0 .. r0 + nr - 1, the first and the last by a
// search (two threads of two waves).  Returns their ends, end[j] = off[r0 + j + 1]: in LDS where nr <= kTileRows, else in
// global memory (thousands of empty rows between two entries).  s_head: two words.  Ends with a barrier.
__device__ __forceinline__ const u32* tile_row_ends(const u32* off, u32 n, u32 e0, u32 e1, u32* s_end, u32* s_head, u32* r0_out, u32* nr_out)
{
    if (threadIdx.x == 0) s_head[0] = first_end_beyond(off + 1, n, e0);
    if (threadIdx.x == 64) s_head[1] = first_end_beyond(off + 1, n, e1 - 1u);
    __syncthreads();
    const u32 r0 = s_head[0], nr = s_head[1] - r0 + 1u;
    if (nr <= kTileRows)
        for (u32 j = threadIdx.x; j < nr; j += kTileThreads) s_end[j] = off[r0 + j + 1];
    __syncthreads();
    *r0_out = r0, *nr_out = nr;
    return nr <= kTileRows ? s_end : off + r0 + 1;
}

// ------------------------------------------------------------------------------------------------ ids
// Gross entry e of gathered row r lies at ro[srow[r]] + (e - G[r]).  Nothing is written but the verdict.  Runs behind the
// check on the same stream: a refused input or 2^32 gross entries (G wrapped) end it before G is read.
__global__ __launch_bounds__(kTileThreads) void sample_ids_kernel(const Gathered g, SampleStatus* st)
{
    SPECK_POISON();
    __shared__ u32 s_end[kTileRows];
    __shared__ u32 s_head[2];
    __shared__ u32 s_go;
    // (one thread asks: another workgroup of this launch may raise the verdict meanwhile, and a workgroup leaves as a whole)
    if (threadIdx.x == 0) s_go = (st->invalid == 0 && st->gross < (1ull << 32)) ? 1u : 0u;
    __syncthreads();
    if (!s_go) return;
    const u64 gross = st->gross;  // (written by the check alone)
    const u64 tiles = (gross + kTile - 1) / kTile;
    bool bad = false;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 e0 = tile * kTile, e1 = std::min<u64>(e0 + kTile, gross);
        u32 r0, nr;
        const u32* end = tile_row_ends(g.G, g.n, (u32)e0, (u32)e1, s_end, s_head, &r0, &nr);
        u32 id[kPer];
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u64 e = e0 + u * kTileThreads + threadIdx.x;
            id[u] = 0u;
            if (e < e1) {
                const u32 r = r0 + first_end_beyond(end, nr, (u32)e);
                id[u] = g.col[g.ro[g.srow[r]] + ((u32)e - g.G[r])];
            }
        }
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) bad |= id[u] >= g.cols;  // (an idle slot holds 0 -- and cols >= 1 wherever an entry exists)
        __syncthreads();  // the next tile overwrites the ends
    }
    if (bad) st->invalid = 1;
}

// ------------------------------------------------------------------------------------------------ mode 1
template <typename T>
__global__ __launch_bounds__(kTileThreads) void sample_draw_kernel(const Gathered g, const T* __restrict__ a_val, u32 nnz_out,
                                                                   u32* __restrict__ c_col, T* __restrict__ c_val)
{
    SPECK_POISON();
    __shared__ u32 s_end[kTileRows];
    __shared__ u32 s_head[2];
    const u64 e0 = u64(blockIdx.x) * kTile, e1 = std::min<u64>(e0 + kTile, nnz_out);
    u32 r0, nr;
    const u32* end = tile_row_ends(g.new_ro, g.n, (u32)e0, (u32)e1, s_end, s_head, &r0, &nr);
    u32 src[kPer];
#pragma unroll
    for (u32 u = 0; u < kPer; ++u) {
        const u64 e = e0 + u * kTileThreads + threadIdx.x;
        src[u] = 0u;
        if (e < e1) {
            const u32 r = r0 + first_end_beyond(end, nr, (u32)e);  // (a row without a draw ends where it starts: never found)
            const u64 key = key_at(row_key_of(g, r), (u32)e - g.new_ro[r]);
            src[u] = g.ro[g.srow[r]] + (u32)__umul64hi(key, (u64)g.glen[r]);
        }
    }
    u32 id[kPer];
    T v[kPer];
#pragma unroll
    for (u32 u = 0; u < kPer; ++u) {
        const u64 e = e0 + u * kTileThreads + threadIdx.x;
        id[u] = 0u;
        v[u] = T(0);
        if (e < e1) {
            id[u] = g.col[src[u]];
            v[u] = a_val[src[u]];
        }
    }
#pragma unroll
    for (u32 u = 0; u < kPer; ++u) {
        const u64 e = e0 + u * kTileThreads + threadIdx.x;
        if (e < e1) {
            c_col[e] = id[u];
            c_val[e] = v[u];
        }
    }
}

// ------------------------------------------------------------------------------------------------ mode 0: rows kept whole
// The entries of the tile's rows of at most k entries, numbered through: entry j of them belongs to the row whose end (an
// inclusive scan of the lengths, LDS) is the first beyond j; s_src / s_dst turn j into its place in A's and in C's buffers.
template <typename T>
__global__ __launch_bounds__(kCopyTileRows) void sample_copy_kernel(const Gathered g, const T* __restrict__ a_val, u32* __restrict__ c_col,
                                                                    T* __restrict__ c_val)
{
    SPECK_POISON();
    __shared__ u32 s_end[kCopyTileRows], s_src[kCopyTileRows], s_dst[kCopyTileRows];
    __shared__ u32 s_scan[kCopyTileRows / 64 + 1];
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kCopyTileRows;
    const u32 nr = min(kCopyTileRows, g.n - r0);
    u32 a = 0, len = 0, to = 0;
    if (t < nr) {
        len = g.glen[r0 + t];
        to = g.new_ro[r0 + t];
        if (len > g.k) len = 0;  // (a class kernel's row)
        if (len) a = g.ro[g.srow[r0 + t]];
    }
    u32 total;
    const u32 ex = block_exclusive_scan<kCopyTileRows>(len, s_scan, &total);
    s_end[t] = ex + len;
    s_src[t] = a - ex;  // (modulo 2^32: the sum with j is the place)
    s_dst[t] = to - ex;
    __syncthreads();
    for (u32 j0 = 0; j0 < total; j0 += kCopyTileRows * kPer) {
        u32 r[kPer], c[kPer];
        T v[kPer];
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 j = j0 + u * kCopyTileRows + t;
            r[u] = j < total ? first_end_beyond(s_end, nr, j) : 0u;
            c[u] = 0u;
            v[u] = T(0);
            if (j < total) {
                c[u] = g.col[s_src[r[u]] + j];
                v[u] = a_val[s_src[r[u]] + j];
            }
        }
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 j = j0 + u * kCopyTileRows + t;
            if (j < total) {
                c_col[s_dst[r[u]] + j] = c[u];
                c_val[s_dst[r[u]] + j] = v[u];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ mode 0: group rows
// Entry p of the row lies in lane p % L, register p / L of its group.  Every lane reads the row's keys from LDS one after
// the other -- the lanes of a group read one address: a broadcast -- and counts for each of its entries the entries that
// beat it: a larger rank key (a smaller key), or an equal one in front.  Kept: fewer than k.
template <typename T, u32 L>
__global__ __launch_bounds__(256) void sample_group_kernel(const Gathered g, const T* __restrict__ a_val, const u32* __restrict__ lists,
                                                           u32* __restrict__ c_col, T* __restrict__ c_val, const SampleStatus* __restrict__ st)
{
    SPECK_POISON();
    constexpr u32 NG = 256 / L, NP = kPer * L;
    constexpr u32 LIST = L == 8 ? LIST_G8 : L == 16 ? LIST_G16 : L == 32 ? LIST_G32 : LIST_G64;
    __shared__ u64 s_key[NG * NP];
    const u32 gl = threadIdx.x % L, gid = threadIdx.x / L;
    const u32 gshift = lane_id() & ~(L - 1u);  // the group's first lane in its wave
    const u64 gmask = L == 64 ? ~0ull : ((1ull << L) - 1ull);
    u64* mine = s_key + gid * NP;
    const u32 n_list = st->cnt[LIST];
    const u32 k = g.k;
    // (whole waves: a group without a row runs the trip with n = 0 -- the ballots below are the wave's)
    for (u32 e0 = blockIdx.x * NG; e0 < n_list; e0 += gridDim.x * NG) {
        const u32 e = e0 + gid;
        u32 a0 = 0, n = 0, o0 = 0;
        u64 rk = 0;
        if (e < n_list) {
            const u32 row = *two_sided_at(lists, g.n, LIST, e);
            a0 = g.ro[g.srow[row]];
            n = min(g.glen[row], NP);
            o0 = g.new_ro[row];
            rk = row_key_of(g, row);
        }
        u64 key[kPer];
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 p = u * L + gl;
            key[u] = 0;
            if (p < n) {
                key[u] = rank_key_at(rk, p);
                mine[p] = key[u];
            }
        }
        wave_lds_fence();
        u32 beat[kPer] = {0, 0, 0, 0};
        for (u32 q = 0; q < n; ++q) {
            const u64 other = mine[q];
#pragma unroll
            for (u32 u = 0; u < kPer; ++u) beat[u] += (other > key[u] || (other == key[u] && q < u * L + gl)) ? 1u : 0u;
        }
        u32 placed = 0;
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 p = u * L + gl;
            const bool kept = p < n && beat[u] < k;
            const u64 m = (__ballot(kept) >> gshift) & gmask;
            if (kept) {
                const u32 to = o0 + placed + (u32)__popcll(m & ((1ull << gl) - 1ull));
                c_col[to] = g.col[a0 + p];
                c_val[to] = a_val[a0 + p];
            }
            placed += (u32)__popcll(m);
        }
        wave_lds_fence();  // the next row overwrites the keys
    }
}

// ------------------------------------------------------------------------------------------------ mode 0: LDS rows, long rows
// an entry of the pass's candidates counts in the bin of its digit: ONE LDS atomic where the wave's candidates share the
// digit (the later passes: few candidates, the upper bytes shared), one per lane elsewhere (the first pass: the keys are
// uniform over the bins).  Whole waves.
__device__ __forceinline__ void histogram_add(u32* s_hist, bool on, u32 digit)
{
    const u64 m = __ballot(on);
    if (m == 0) return;
    const u32 leader = (u32)__ffsll((long long)m) - 1u;
    const u32 d0 = (u32)__shfl((int)digit, (int)leader);
    if (__ballot(on && digit == d0) == m) {
        if (lane_id() == leader) atomicAdd(&s_hist[d0], (u32)__popcll(m));
    } else if (on) atomicAdd(&s_hist[digit], 1u);
}

template <typename T, u32 kThreads, bool kLds>
__global__ __launch_bounds__(kThreads) void sample_row_kernel(const Gathered g, const T* __restrict__ a_val, const u32* __restrict__ lists,
                                                              u32* __restrict__ c_col, T* __restrict__ c_val,
                                                              const SampleStatus* __restrict__ st)
{
    SPECK_POISON();
    constexpr u32 LIST = kLds ? LIST_LDS : LIST_LONG;
    static_assert(kThreads >= 256 && kThreads <= 1024, "a thread per bin; a scan's counts fit 16 bits");
    __shared__ u64 s_key[kLds ? kLdsMax : 1];
    __shared__ u32 s_hist[256];
    __shared__ u32 s_scan[kThreads / 64 + 1];
    __shared__ u32 s_sel[3];
    const u32 t = threadIdx.x;
    const u32 n_list = st->cnt[LIST];
    const u32 k = g.k;
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(lists, g.n, LIST, e);
        const u32 a0 = g.ro[g.srow[row]], o0 = g.new_ro[row];
        const u32 n = kLds ? min(g.glen[row], kLdsMax) : g.glen[row];
        const u64 rk = row_key_of(g, row);
        if (kLds)
            for (u32 i = t; i < n; i += kThreads) s_key[i] = rank_key_at(rk, i);
        // ---- the k-th key: `prefix` = its bytes above `shift`, `need` = the entries still to take among the keys that
        // share them (every key with larger upper bytes is taken)
        u64 prefix = 0;
        u32 need = k, shift = 64, bin_cnt = 0;
        do {
            const bool first = shift == 64;
            const u32 upper = first ? 0u : shift;  // the candidates: key >> upper == prefix
            shift -= 8;
            if (t < 256) s_hist[t] = 0;
            __syncthreads();  // (and the keys are in LDS)
            for (u64 i0 = 0; i0 < n; i0 += u64(kThreads) * kPer) {
                u64 key[kPer];
                bool ok[kPer];
#pragma unroll
                for (u32 u = 0; u < kPer; ++u) {
                    const u64 i = i0 + u * kThreads + t;
                    ok[u] = i < n;
                    key[u] = 0;
                    if (ok[u]) key[u] = kLds ? s_key[i] : rank_key_at(rk, i);
                }
#pragma unroll
                for (u32 u = 0; u < kPer; ++u)
                    histogram_add(s_hist, ok[u] && (first || (key[u] >> upper) == prefix), (u32)(key[u] >> shift) & 255u);
            }
            __syncthreads();
            // bin 255 - t: the candidates in the bins above it are those of the threads before me
            const u32 mine = t < 256 ? s_hist[255 - t] : 0u;
            u32 total;
            const u32 above = block_exclusive_scan<kThreads>(mine, s_scan, &total);
            if (t < 256 && above < need && need <= above + mine) s_sel[0] = 255 - t, s_sel[1] = above, s_sel[2] = mine;
            __syncthreads();
            prefix = (prefix << 8) | u64(s_sel[0]);
            need -= s_sel[1];
            bin_cnt = s_sel[2];
        } while (shift != 0 && bin_cnt != need);  // (the whole bin is needed: nothing is left to narrow)
        // keep key > tau, and the first tq of key == tau
        u64 tau = prefix;
        u32 tq = need;
        if (shift != 0) tau = (prefix << shift) - 1u, tq = 0;  // every key from prefix << shift on (> 0: fewer than n are kept)
        // ---- the ordered walk: one packed scan (low half: key > tau, high half: key == tau) per kThreads entries
        u32 carry_gt = 0, carry_eq = 0;
        for (u64 i0 = 0; i0 < n; i0 += u64(kThreads) * kPer) {
            u64 key[kPer];
            bool ok[kPer];
#pragma unroll
            for (u32 u = 0; u < kPer; ++u) {
                const u64 i = i0 + u * kThreads + t;
                ok[u] = i < n;
                key[u] = 0;
                if (ok[u]) key[u] = kLds ? s_key[i] : rank_key_at(rk, i);
            }
#pragma unroll
            for (u32 u = 0; u < kPer; ++u) {
                const u64 i = i0 + u * kThreads + t;
                const bool gt = ok[u] && key[u] > tau, eq = ok[u] && key[u] == tau;
                u32 total;
                const u32 ex = block_exclusive_scan<kThreads>((gt ? 1u : 0u) | (eq ? 0x10000u : 0u), s_scan, &total);
                const u32 gt_before = carry_gt + (ex & 0xFFFFu), eq_before = carry_eq + (ex >> 16);
                if (gt || (eq && eq_before < tq)) {
                    const u32 to = o0 + gt_before + min(eq_before, tq);
                    c_col[to] = g.col[a0 + i];
                    c_val[to] = a_val[a0 + i];
                }
                carry_gt += total & 0xFFFFu;
                carry_eq += total >> 16;
            }
        }
        __syncthreads();  // the next row overwrites the keys
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename I, typename T>
int sample_run(SampleScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_sample_params* p, speck_dcsr* C, speck_sample_info* info,
               COut* out)
{
    const u32 rows = (u32)A->rows, n = (u32)p->n_rows;
    const u64 nnz = A->nnz;
    const bool draw = p->mode == SPECK_SAMPLE_WITH_REPLACEMENT;
    const u32 k = (u32)std::min<u64>(p->k, 0xFFFFFFFFull);  // (a row holds fewer than 2^32 entries: such a k cuts none)
    const u64 k_draw = std::min<u64>(p->k, 1ull << 32);     // (2^32 draws of one row are refused: the sum of 2^27 such rows fits 64 bits)

    // status | lists (three regions of n words) | source row | gathered length | G | output length | new row offsets | scan sums
    const size_t list_bytes = up256(size_t(3) * n * 4), row_bytes = up256((size_t(n) + 1) * 4);
    const size_t sum_bytes = up256(size_t((n + 1023) / 1024 + 1) * 4);
    int rc = sc->fixed.ensure(256 + list_bytes + 5 * row_bytes + sum_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* fb = static_cast<unsigned char*>(sc->fixed.p);
    static_assert(sizeof(SampleStatus) <= 256, "status block");
    SampleStatus* st = reinterpret_cast<SampleStatus*>(fb);
    u32* lists = reinterpret_cast<u32*>(fb + 256);
    u32* srow = reinterpret_cast<u32*>(fb + 256 + list_bytes);
    u32* glen = reinterpret_cast<u32*>(fb + 256 + list_bytes + row_bytes);
    u32* G = reinterpret_cast<u32*>(fb + 256 + list_bytes + 2 * row_bytes);
    u32* row_cnt = reinterpret_cast<u32*>(fb + 256 + list_bytes + 3 * row_bytes);
    u32* new_ro = reinterpret_cast<u32*>(fb + 256 + list_bytes + 4 * row_bytes);
    u32* block_sums = reinterpret_cast<u32*>(fb + 256 + list_bytes + 5 * row_bytes);

    // ---- the verdict on A's offsets, the indices and the ids of the gathered rows, nnz(C) and the lists: read before
    // anything of C is allocated or written
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SampleStatus), s));
    SPECK_LAUNCH(sample_check_kernel<I>, dim3(grid_of((std::max<u64>(rows, n) + 255) / 256, kCheckGrid)), dim3(256), 0, s, A->row_offsets,
                 A->col_ids, A->data, (u32)sizeof(T), static_cast<const I*>(p->d_row_index), rows, n, nnz, k, k_draw, p->mode, sc->group_max,
                 sc->lds_max, srow, glen, row_cnt, lists, st);
    const Gathered g{A->row_offsets, A->col_ids, srow, glen, G, new_ro, n, (u32)A->cols, k, p->seed, p->row_base};
    if (n) {
        // (on a refused input or a sum of 2^32 or more the offsets are whatever the words add up to: nothing is addressed
        //  through them -- the id pass ends at once, the host refuses the call)
        launch_exclusive_scan(s, CountArray{glen}, n, block_sums, G, nullptr);
        launch_exclusive_scan(s, CountArray{row_cnt}, n, block_sums, new_ro, nullptr);
        if (nnz) {
            // a list of all rows gathers nnz entries; an index list may gather any number: the grid strides
            const u64 tiles = p->d_row_index ? kIdsGrid : (nnz + kTile - 1) / kTile;
            SPECK_LAUNCH(sample_ids_kernel, dim3(grid_of(tiles, kIdsGrid)), dim3(kTileThreads), 0, s, g, st);
        }
    }
    SampleStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    // (2^32: the offsets wrapped, nothing has read them; repeats in the list can make the gathered rows pass the copy's limit too)
    if (h.gross > kSampleEntriesMax || h.nnz_out >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (n == 0) return publish_empty_c(C, A->cols, sizeof(T), s, out);

    // ---- C
    const u64 nnz_out = h.nnz_out;
    rc = prepare_c(C, n, nnz_out, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    if (nnz_out) {
        const T* val = static_cast<const T*>(A->data);
        u32* c_col = out->col;
        T* c_val = static_cast<T*>(out->val);
        if (draw)
            SPECK_LAUNCH(sample_draw_kernel<T>, dim3((u32)((nnz_out + kTile - 1) / kTile)), dim3(kTileThreads), 0, s, g, val, (u32)nnz_out,
                         c_col, c_val);
        else {
            if (h.rows_cut < n)
                SPECK_LAUNCH(sample_copy_kernel<T>, dim3((n + kCopyTileRows - 1) / kCopyTileRows), dim3(kCopyTileRows), 0, s, g, val, c_col,
                             c_val);
            if (h.cnt[LIST_G8])
                SPECK_LAUNCH((sample_group_kernel<T, 8>), dim3(grid_of((h.cnt[LIST_G8] + 31) / 32, kGroupGrid)), dim3(256), 0, s, g, val, lists,
                             c_col, c_val, st);
            if (h.cnt[LIST_G16])
                SPECK_LAUNCH((sample_group_kernel<T, 16>), dim3(grid_of((h.cnt[LIST_G16] + 15) / 16, kGroupGrid)), dim3(256), 0, s, g, val, lists,
                             c_col, c_val, st);
            if (h.cnt[LIST_G32])
                SPECK_LAUNCH((sample_group_kernel<T, 32>), dim3(grid_of((h.cnt[LIST_G32] + 7) / 8, kGroupGrid)), dim3(256), 0, s, g, val, lists,
                             c_col, c_val, st);
            if (h.cnt[LIST_G64])
                SPECK_LAUNCH((sample_group_kernel<T, 64>), dim3(grid_of((h.cnt[LIST_G64] + 3) / 4, kGroupGrid)), dim3(256), 0, s, g, val, lists,
                             c_col, c_val, st);
            if (h.cnt[LIST_LDS])
                SPECK_LAUNCH((sample_row_kernel<T, 256, true>), dim3(grid_of(h.cnt[LIST_LDS], kLdsGrid)), dim3(256), 0, s, g, val, lists, c_col,
                             c_val, st);
            if (h.cnt[LIST_LONG])
                SPECK_LAUNCH((sample_row_kernel<T, 1024, false>), dim3(grid_of(h.cnt[LIST_LONG], kLongGrid)), dim3(1024), 0, s, g, val, lists,
                             c_col, c_val, st);
        }
    }
    rc = finish_rows(s, new_ro, n, A->cols, nnz_out, C, out);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->rows_out = n;
        info->rows_empty = h.rows_empty;
        info->rows_cut = h.rows_cut;
        info->gross = h.gross;
        info->nnz_out = nnz_out;
        info->max_row_entries = h.max_row;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"sample lists, lengths and offsets", "sample temporaries", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int sample_impl(speck_config* cfg, const speck_dcsr* A, const speck_sample_params* p, speck_dcsr* C, speck_sample_info* info)
{
    if (!A || !p || !C) return SPECK_ERR_INVALID;
    if (p->mode != SPECK_SAMPLE_WITHOUT_REPLACEMENT && p->mode != SPECK_SAMPLE_WITH_REPLACEMENT) return SPECK_ERR_INVALID;
    if (p->index_bytes != 4 && p->index_bytes != 8) return SPECK_ERR_INVALID;
    if (p->row_base > (1ull << 62)) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || p->n_rows > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    // (sample_copy_kernel numbers the kept entries of a tile of 256 rows in 32 bits and steps by 1024)
    if (A->nnz > kSampleEntriesMax) return SPECK_ERR_NNZ_OVERFLOW;
    if (!csr_args_ok(A, true) || (A->nnz && (A->rows == 0 || A->cols == 0))) return SPECK_ERR_INVALID;
    if (!p->d_row_index && p->n_rows != A->rows) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A)) return SPECK_ERR_INVALID;
    // the index against A's and C's buffers as far as the host knows their place (the entries of a view: the check pass)
    const void* theirs[6] = {A->data, A->col_ids, A->row_offsets, C->data, C->col_ids, C->row_offsets};
    const u64 their_len[6] = {A->nnz * sizeof(T), A->nnz * 4, (A->rows + 1) * 4, C->nnz * sizeof(T), C->nnz * 4, (C->rows + 1) * 4};
    for (int b = 0; b < 6; ++b)
        if (spans_overlap(p->d_row_index, p->n_rows * p->index_bytes, theirs[b], their_len[b])) return SPECK_ERR_INVALID;
    if (info) *info = speck_sample_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, sample_scratch, C, info, kGuardNames, " by the sampling", [&](SampleScratch* sc, hipStream_t s, COut* out) {
        return p->index_bytes == 8 ? sample_run<u64, T>(sc, s, A, p, C, info, out) : sample_run<u32, T>(sc, s, A, p, C, info, out);
    });
}

}  // namespace

extern "C" {

int speck_sample_f64(speck_config* cfg, const speck_dcsr* A, const speck_sample_params* p, speck_dcsr* C, speck_sample_info* info)
{
    return sample_impl<double>(cfg, A, p, C, info);
}

int speck_sample_f32(speck_config* cfg, const speck_dcsr* A, const speck_sample_params* p, speck_dcsr* C, speck_sample_info* info)
{
    return sample_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
