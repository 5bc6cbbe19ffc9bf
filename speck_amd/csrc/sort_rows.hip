// sort_rows.hip -- speck_sort_rows_*: the rows of a device CSR sorted in place by column id (stable), optionally with
// equal columns merged.  What makes a matrix that was produced ON the device acceptable to speck_multiply_* (whose input
// check wants strictly ascending rows).  The reference has no counterpart: its host loader sorts (source/CSR.cpp:173-212).
//
//   sort_classify_kernel   one streaming pass over row_offsets and col_ids: the input check (the offset check:
//                          row_tiles.hpp; columns < cols -- no offset is used as an address before it was checked) and,
//                          per row, "strictly ascending?".  Rows that are pass no further; the others go to one of six
//                          lists by length (wave-aggregated atomic cursors: the order inside a list does not matter).
//   sort_reg_kernel<L>     rows of <= 4 L entries, L = 8 / 16 / 32 / 64 lanes per row: the sorting networks of esc.hpp /
//                          esc_wide.hpp on keys (column - smallest column of the row) << 8 | position.  The position makes
//                          the sort stable and gathers the value (staged in LDS by position).  A row whose column range
//                          does not fit 24 bits is handed on to the LDS list.
//   sort_lds_kernel        one workgroup per row of <= kSortLdsMax entries: bitonic network in LDS on 64-bit keys
//                          column << 32 | position; the values are gathered into registers, a barrier, then stored.
//   sort_global_kernel     one workgroup per longer row: stable LSD radix sort (8-bit digits, ranks from ballots as in the
//                          transpose's radix_scatter_kernel, tiles taken in order) between the row and a temporary.
//   compaction             (SUM_DUPLICATES, when a row shrank) row lengths minus duplicates -> the shared scan
//                          (scan.hpp) -> the runs summed in double while the rows move to a temporary -> copied back.
// The host side stands on host_common.hpp and side_call.hpp (the status read-back, the guard check after the call); the
// frame of the call is its own: M is sorted in place, no C is handed over, and a refused call keeps what it told `info`.
// Every kernel that writes M starts after the host has read the verdict of the classifying pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "esc.hpp"
#include "esc_wide.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "side_call.hpp"
#include "sort_rows.hpp"

using namespace speck;

namespace {

constexpr u32 kSortRegMax = SPECK_SORT_REG_MAX, kSortLdsMax = SPECK_SORT_LDS_MAX;
constexpr u32 kSortRangeMax = (1u << 24) - 1u;  // column range a register key holds (the all-ones key means "no entry")
enum { LIST_R8 = 0, LIST_R16, LIST_R32, LIST_R64, LIST_LDS, LIST_GLOBAL, SORT_LISTS };

struct SortStatus {
    u32 invalid;           // the input check failed
    u32 in_order;          // rows strictly ascending
    u32 cnt[SORT_LISTS];   // list lengths
    u32 deferred;          // rows a register kernel handed on to the LDS list
    u32 base;              // row_offsets[0]
    unsigned long long dups;            // entries whose column an earlier entry of their row holds
    unsigned long long global_entries;  // entries of the rows in LIST_GLOBAL
    unsigned long long temp_cursor;     // next free entry of the long-row temporaries
};

// (the six lists share three regions of `rows` words: two_sided_at, device_common.hpp)

// ------------------------------------------------------------------------------------------------ check + classify
// 128 or 512 rows (the host picks by the average row length: a tile should hold enough entries to pay for its barriers,
// and there should be enough tiles for the machine) and 512 threads per workgroup: the tile's entries are walked a thread
// per entry, four loads in flight per thread.  Which row an entry belongs to matters only where it is not above its
// predecessor: a binary search over the tile's offsets (LDS) there, nowhere else -- on a canonical matrix that is one
// search per row boundary at most.
constexpr u32 kClassifyThreads = 512, kClassifyUnroll = 4;

template <u32 kTileRows>
__global__ __launch_bounds__(kClassifyThreads) void sort_classify_kernel(const u32* __restrict__ ro, const u32* __restrict__ col,
                                                                         u32 rows, u32 cols, u64 nnz, u32 reg_max, u32 lds_max,
                                                                         u32* __restrict__ lists, SortStatus* __restrict__ st)
{
    SPECK_POISON();
    static_assert(kTileRows <= kClassifyThreads, "a thread per row classifies");
    __shared__ u32 s_ro[kTileRows + 1];
    __shared__ u32 s_flag[kTileRows];
    __shared__ u32 s_bad;
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kTileRows;
    const u32 nr = min(kTileRows, rows - r0);
    const u32 base = ro[0];
    if (t == 0) s_bad = 0;
    if (t == 0 && blockIdx.x == 0) st->base = base;
    if (t < kTileRows) s_flag[t] = 0;
    __syncthreads();
    tile_offsets_load<kClassifyThreads>(ro, r0, nr, base, nnz, s_ro, &s_bad);
    __syncthreads();
    if (tile_offsets_descend(s_ro, nr)) s_bad = 1;
    __syncthreads();
    if (s_bad) {  // (nothing of col_ids is addressed through such offsets)
        if (t == 0) st->invalid = 1;
        return;
    }
    // the tile's entries: offsets are monotone and inside [base, base + nnz] here
    const u64 lo = s_ro[0], hi = s_ro[nr];
    bool bad_col = false;
    u64 seen_lo = 0, seen_hi = 0;  // entries of the row this thread found out of order last: flagged already
    for (u64 i0 = lo + t; i0 < hi; i0 += kClassifyThreads * kClassifyUnroll) {
        u32 c[kClassifyUnroll], p[kClassifyUnroll];
#pragma unroll
        for (u32 k = 0; k < kClassifyUnroll; ++k) {
            const u64 i = i0 + k * kClassifyThreads;
            c[k] = i < hi ? col[i] : 0u;
            p[k] = (i < hi && i > lo) ? col[i - 1] : 0u;  // (entry `lo` starts a row: nothing in front of it is read)
        }
#pragma unroll
        for (u32 k = 0; k < kClassifyUnroll; ++k) {
            const u64 i = i0 + k * kClassifyThreads;
            if (i >= hi) continue;
            bad_col |= c[k] >= cols;
            if (i > lo && p[k] >= c[k]) {
                if (i < seen_lo || i >= seen_hi) {  // (a long row: the row of the thread's previous find, as a rule)
                    const u32 a = first_end_beyond(s_ro + 1, nr, i);  // the row of entry i
                    if (i > s_ro[a]) {  // (not the first entry of its row)
                        seen_lo = s_ro[a], seen_hi = s_ro[a + 1];
                        if (!s_flag[a]) s_flag[a] = 1;
                    }
                }
            }
        }
    }
    if (bad_col) st->invalid = 1;
    __syncthreads();
    int cls = -2;  // no row
    u32 len = 0;
    if (t < nr) {
        len = s_ro[t + 1] - s_ro[t];
        if (!s_flag[t]) cls = -1;
        else if (len <= reg_max && len <= kSortRegMax) cls = len <= 32 ? LIST_R8 : len <= 64 ? LIST_R16 : len <= 128 ? LIST_R32 : LIST_R64;
        else cls = len <= lds_max ? LIST_LDS : LIST_GLOBAL;
    }
    const u32 lane = lane_id();
    {
        const u64 m = __ballot(cls == -1);
        if (m && lane == (u32)__ffsll((long long)m) - 1u) atomicAdd(&st->in_order, (u32)__popcll(m));
    }
#pragma unroll
    for (int k = 0; k < SORT_LISTS; ++k) {
        const u64 m = __ballot(cls == k);
        if (m == 0) continue;
        const u32 leader = (u32)__ffsll((long long)m) - 1u;
        u32 first = 0;
        if (lane == leader) first = atomicAdd(&st->cnt[k], (u32)__popcll(m));
        first = (u32)__shfl((int)first, (int)leader);
        if (cls == k) *two_sided_at(lists, rows, k, first + (u32)__popcll(m & lanemask_lt())) = r0 + t;
    }
    if (cls == LIST_GLOBAL) atomicAdd(&st->global_entries, (unsigned long long)len);
}

// ------------------------------------------------------------------------------------------------ register class
template <u32 L>
__device__ __forceinline__ u32 group_min(u32 v)
{
#pragma unroll
    for (u32 m = L / 2; m; m >>= 1) v = min(v, (u32)__shfl_xor((int)v, (int)m, (int)L));
    return v;
}
template <u32 L>
__device__ __forceinline__ u32 group_max(u32 v)
{
#pragma unroll
    for (u32 m = L / 2; m; m >>= 1) v = max(v, (u32)__shfl_xor((int)v, (int)m, (int)L));
    return v;
}

template <typename T, u32 L>
__global__ __launch_bounds__(256) void sort_reg_kernel(const u32* __restrict__ ro, u32* col, T* val, u32 rows, u32* lists,
                                                       SortStatus* st, u32* __restrict__ row_dups)
{
    SPECK_POISON();
    constexpr u32 NG = 256 / L, NP = 4 * L, PER = kEscPerLane;
    constexpr u32 K = L == 8 ? LIST_R8 : L == 16 ? LIST_R16 : L == 32 ? LIST_R32 : LIST_R64;
    __shared__ T s_val[NG * NP];  // the values of each group's row, by input position
    const SubWave<L> g;
    const u32 gl = g.lane, gid = threadIdx.x / L;
    T* mine = s_val + gid * NP;
    const u32 n_list = st->cnt[K];
    for (u32 e = blockIdx.x * NG + gid; e < n_list; e += gridDim.x * NG) {
        const u32 row = *two_sided_at(lists, rows, K, e);
        const u32 a0 = ro[row], n = min(ro[row + 1] - a0, NP);
        u32 c[PER];
        T v[PER];
        u32 cmin = 0xFFFFFFFFu, cmax = 0;
#pragma unroll
        for (u32 u = 0; u < PER; ++u) {
            const u32 p = u * L + gl;
            c[u] = 0;
            v[u] = T(0);
            if (p < n) {
                c[u] = col[a0 + p];
                v[u] = val[a0 + p];
                cmin = min(cmin, c[u]);
                cmax = max(cmax, c[u]);
            }
        }
        cmin = group_min<L>(cmin);
        cmax = group_max<L>(cmax);
        if (cmax - cmin >= kSortRangeMax) {  // the key does not hold the row's columns: the LDS class takes it
            if (gl == 0) {
                *two_sided_at(lists, rows, LIST_LDS, atomicAdd(&st->cnt[LIST_LDS], 1u)) = row;
                atomicAdd(&st->deferred, 1u);
            }
            continue;
        }
        u32 key[PER];
#pragma unroll
        for (u32 u = 0; u < PER; ++u) {
            const u32 p = u * L + gl;
            key[u] = kEscInvalid;
            if (p < n) {
                key[u] = ((c[u] - cmin) << 8) | p;
                mine[p] = v[u];
            }
        }
        wave_lds_fence();
        if constexpr (L <= 16) esc_sort<L>(key, gl);
        else esc_sort_wide<L>(key, gl);
        // element i = lane * 4 + register of the sorted row; every load of the row has completed (the keys depend on them)
        const u32 prev_key = (u32)__shfl_up((int)key[PER - 1], 1, (int)L);
        u32 dups = 0;
#pragma unroll
        for (u32 r = 0; r < PER; ++r) {
            const u32 i = gl * PER + r;
            if (i < n) {
                const u32 before = r ? key[r - 1] : prev_key;
                dups += (i != 0 && (before >> 8) == (key[r] >> 8)) ? 1u : 0u;
                col[a0 + i] = (key[r] >> 8) + cmin;
                val[a0 + i] = mine[key[r] & 255u];
            }
        }
        dups = g.reduce_add(dups, nullptr);
        if (gl == 0 && dups) {
            atomicAdd(&st->dups, (unsigned long long)dups);
            if (row_dups) row_dups[row] = dups;
        }
        wave_lds_fence();  // the next row overwrites the values
    }
}

// ------------------------------------------------------------------------------------------------ LDS class
// Keys column << 32 | position: distinct, so the (unstable) network gives the stable order.  8 B of LDS per entry: 32 KiB
// for the longest row, five workgroups resident per CU.  The values do not pass through LDS: each thread gathers the (up
// to 16) values of the places it will store, all threads meet at a barrier, then they store.
template <typename T>
__global__ __launch_bounds__(256) void sort_lds_kernel(const u32* __restrict__ ro, u32* col, T* val, u32 rows, u32* lists,
                                                       SortStatus* st, u32* __restrict__ row_dups)
{
    SPECK_POISON();
    constexpr u32 PER = kSortLdsMax / 256;
    __shared__ u64 s_key[kSortLdsMax];
    __shared__ u32 s_dups;
    const u32 t = threadIdx.x;
    const u32 n_list = st->cnt[LIST_LDS];
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(lists, rows, LIST_LDS, e);
        const u32 a0 = ro[row], n = min(ro[row + 1] - a0, kSortLdsMax);
        u32 n2 = 2;
        while (n2 < n) n2 <<= 1;
        if (t == 0) s_dups = 0;
        for (u32 i = t; i < n2; i += 256) s_key[i] = i < n ? (u64(col[a0 + i]) << 32) | i : ~0ull;
        __syncthreads();
        for (u32 k = 2; k <= n2; k <<= 1)
            for (u32 j = k >> 1; j; j >>= 1) {
                for (u32 p = t; p < n2 / 2; p += 256) {
                    const u32 i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), l = i | j;
                    const u64 x = s_key[i], y = s_key[l];
                    if ((x > y) == ((i & k) == 0)) {
                        s_key[i] = y;
                        s_key[l] = x;
                    }
                }
                __syncthreads();
            }
        T v[PER];
        u32 dups = 0;
#pragma unroll
        for (u32 u = 0; u < PER; ++u) {
            const u32 i = u * 256 + t;
            v[u] = T(0);
            if (i < n) {
                const u64 k = s_key[i];
                v[u] = val[a0 + (u32)k];
                dups += (i != 0 && (u32)(s_key[i - 1] >> 32) == (u32)(k >> 32)) ? 1u : 0u;
            }
        }
        if (dups) atomicAdd(&s_dups, dups);
        __syncthreads();  // every value of the row is in a register
#pragma unroll
        for (u32 u = 0; u < PER; ++u) {
            const u32 i = u * 256 + t;
            if (i < n) {
                col[a0 + i] = (u32)(s_key[i] >> 32);
                val[a0 + i] = v[u];
            }
        }
        __syncthreads();
        if (t == 0 && s_dups) {
            atomicAdd(&st->dups, (unsigned long long)s_dups);
            if (row_dups) row_dups[row] = s_dups;
        }
        __syncthreads();  // the next row overwrites the keys and the counter
    }
}

// ------------------------------------------------------------------------------------------------ global class
// One workgroup per row; (column, position) pairs travel between the row's place in col_ids + one position buffer and a
// second pair of buffers, one 8-bit digit per pass, least significant first.  Tiles of 256 x 8 entries are taken in order
// and ranked as in radix_scatter_kernel (extras.hip): the rank of a key among the equal digits before it = what the waves
// before mine hold + the running count of my wave + the lanes before me in the step that hold my digit.  At the end the
// columns are copied home if they rest in the temporary, and the values are gathered through a copy of the row's values.
// Serves a handful of rows: correct first.
constexpr u32 kGItems = 8, kGTile = 256 * kGItems;

template <typename T>
__global__ __launch_bounds__(256) void sort_global_kernel(const u32* __restrict__ ro, u32* col, T* val, u32 rows, u32* lists,
                                                          SortStatus* st, u32* __restrict__ row_dups, u32* tmp_key, u32* tmp_pos0,
                                                          u32* tmp_pos1, T* tmp_val, u64 tmp_entries, u32 bits)
{
    SPECK_POISON();
    constexpr int NW = 4;
    __shared__ u32 s_base[256];
    __shared__ u32 s_wave[NW][256];
    __shared__ u32 s_scan[NW + 1];
    __shared__ u64 s_off;
    __shared__ u32 s_dups;
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u32 n_list = st->cnt[LIST_GLOBAL];
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(lists, rows, LIST_GLOBAL, e);
        const u32 a0 = ro[row], n = ro[row + 1] - a0;
        if (t == 0) {
            s_off = atomicAdd(&st->temp_cursor, (unsigned long long)n);
            s_dups = 0;
        }
        __syncthreads();
        const u64 off = s_off;
        if (off + n > tmp_entries) {  // (cannot happen: the temporaries hold the entries of every listed row)
            __syncthreads();
            continue;
        }
        u32* keys[2] = {col + a0, tmp_key + off};
        u32* poss[2] = {tmp_pos0 + off, tmp_pos1 + off};
        int cur = 0;
        for (u32 shift = 0; shift < bits; shift += 8) {
            const u32* kin = keys[cur];
            const u32* pin = poss[cur];
            u32* kout = keys[cur ^ 1];
            u32* pout = poss[cur ^ 1];
            s_base[t] = 0;
            __syncthreads();
            for (u64 i = t; i < n; i += 256) atomicAdd(&s_base[(kin[i] >> shift) & 255u], 1u);
            __syncthreads();
            u32 total;
            const u32 mine = s_base[t];
            const u32 excl = block_exclusive_scan<256>(mine, s_scan, &total);
            s_base[t] = excl;
            __syncthreads();
            for (u64 t0 = 0; t0 < n; t0 += kGTile) {
#pragma unroll
                for (int w = 0; w < NW; ++w) s_wave[w][t] = 0;
                __syncthreads();
                u32 key[kGItems], pos[kGItems], rank[kGItems];
#pragma unroll
                for (u32 it = 0; it < kGItems; ++it) {
                    const u64 i = t0 + (wid * kGItems + it) * 64 + lane;
                    const bool ok = i < n;
                    key[it] = ok ? kin[i] : 0u;
                    pos[it] = ok ? (shift == 0 ? (u32)i : pin[i]) : 0u;
                    const u32 d = (key[it] >> shift) & 255u;
                    u64 peers = __ballot(ok);
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const u64 m = __ballot((d >> b) & 1u);
                        peers &= ((d >> b) & 1u) ? m : ~m;
                    }
                    const u32 before = s_wave[wid][d];
                    rank[it] = before + (u32)__popcll(peers & lanemask_lt());
                    if (ok && (peers & lanemask_lt()) == 0) s_wave[wid][d] = before + (u32)__popcll(peers);
                    wave_lds_fence();
                }
                __syncthreads();
                {
                    u32 run = s_base[t];
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const u32 cnt = s_wave[w][t];
                        s_wave[w][t] = run;
                        run += cnt;
                    }
                    s_base[t] = run;
                }
                __syncthreads();
#pragma unroll
                for (u32 it = 0; it < kGItems; ++it) {
                    const u64 i = t0 + (wid * kGItems + it) * 64 + lane;
                    if (i < n) {
                        const u32 to = s_wave[wid][(key[it] >> shift) & 255u] + rank[it];
                        kout[to] = key[it];
                        pout[to] = pos[it];
                    }
                }
                __syncthreads();
            }
            __threadfence_block();
            __syncthreads();  // the pass is complete in memory before the next one reads it
            cur ^= 1;
        }
        const u32* ksorted = keys[cur];
        const u32* psorted = poss[cur];
        T* vcopy = tmp_val + off;
        u32 dups = 0;
        for (u64 i = t; i < n; i += 256) {
            vcopy[i] = val[a0 + i];
            dups += (i != 0 && ksorted[i - 1] == ksorted[i]) ? 1u : 0u;
        }
        if (dups) atomicAdd(&s_dups, dups);
        __threadfence_block();
        __syncthreads();
        for (u64 i = t; i < n; i += 256) {
            if (cur) col[a0 + i] = ksorted[i];
            val[a0 + i] = vcopy[psorted[i]];
        }
        __syncthreads();
        if (t == 0 && s_dups) {
            atomicAdd(&st->dups, (unsigned long long)s_dups);
            if (row_dups) row_dups[row] = s_dups;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ compaction
// Rows move LEFT inside one buffer: in parallel that is a read / write race between rows, so the rows go through a
// temporary (new columns, new values: nnz_out entries each) and are copied back with two device-to-device copies; the new
// row offsets are built in a temporary as well and copied over row_offsets last.
// what a row keeps: the count the shared scan (scan.hpp) turns into the new row offsets
struct SortNewLen {
    const u32 *ro, *row_dups;
    __device__ u32 operator()(u32 r) const { return ro[r + 1] - ro[r] - row_dups[r]; }
};

// a wave per row: the first entry of every run of equal columns carries the run's sum to its new place
template <typename T>
__global__ __launch_bounds__(256) void sort_compact_kernel(const u32* __restrict__ ro, const u32* __restrict__ col,
                                                           const T* __restrict__ val, const u32* __restrict__ new_ro, u32 rows,
                                                           u32* __restrict__ out_col, T* __restrict__ out_val)
{
    SPECK_POISON();
    const u32 lane = lane_id();
    const u64 wave = (u64(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const u64 nwaves = (u64(gridDim.x) * blockDim.x) >> 6;
    for (u64 row = wave; row < rows; row += nwaves) {
        const u32 a0 = ro[row], n = ro[row + 1] - a0;
        const u32 o0 = new_ro[row];
        const bool same = new_ro[row + 1] - o0 == n;  // nothing to merge: a copy
        u32 placed = 0;
        for (u64 i0 = 0; i0 < n; i0 += 64) {
            const u64 i = i0 + lane;
            const bool ok = i < n;
            const u32 c = ok ? col[a0 + i] : 0u;
            const bool head = ok && (same || i == 0 || col[a0 + i - 1] != c);
            const u64 m = __ballot(head);
            if (head) {
                Acc<T> s = (Acc<T>)val[a0 + i];
                if (!same)
                    for (u64 j = i + 1; j < n && col[a0 + j] == c; ++j) s += (Acc<T>)val[a0 + j];
                const u32 to = o0 + placed + (u32)__popcll(m & lanemask_lt());
                out_col[to] = c;
                out_val[to] = (T)s;
            }
            placed += (u32)__popcll(m);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int sort_rows_run(SortScratch* sc, hipStream_t s, speck_dcsr* M, int flags, speck_sort_info* info)
{
    const u32 rows = (u32)M->rows, cols = (u32)M->cols;
    const u64 nnz = M->nnz;
    u32* ro = M->row_offsets;
    u32* col = M->col_ids;
    T* val = static_cast<T*>(M->data);
    const bool sum = flags == SPECK_SORT_SUM_DUPLICATES;

    // status | lists (three regions of `rows` words) | duplicates per row (SUM only)
    const size_t list_bytes = up256(size_t(3) * rows * 4), dup_bytes = up256(size_t(rows) * 4);
    int rc = sc->fixed.ensure(256 + list_bytes + dup_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* fb = static_cast<unsigned char*>(sc->fixed.p);
    SortStatus* st = reinterpret_cast<SortStatus*>(fb);
    u32* lists = reinterpret_cast<u32*>(fb + 256);
    u32* row_dups = reinterpret_cast<u32*>(fb + 256 + list_bytes);
    static_assert(sizeof(SortStatus) <= 256, "status block");

    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SortStatus), s));
    if (nnz / rows >= kSortTileLongAvg || rows < kSortTileLongRows)  // (measured: the scircuit stand-in's 171 k short rows want the small tile too)
        SPECK_LAUNCH(sort_classify_kernel<kSortTileRows>, dim3((rows + kSortTileRows - 1) / kSortTileRows), dim3(kClassifyThreads), 0, s,
                     ro, col, rows, cols, nnz, sc->reg_max, sc->lds_max, lists, st);
    else
        SPECK_LAUNCH(sort_classify_kernel<kSortTileRowsLong>, dim3((rows + kSortTileRowsLong - 1) / kSortTileRowsLong),
                     dim3(kClassifyThreads), 0, s, ro, col, rows, cols, nnz, sc->reg_max, sc->lds_max, lists, st);
    SortStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;

    u64 to_sort = 0;
    for (int k = 0; k < SORT_LISTS; ++k) to_sort += h.cnt[k];
    if (info) info->rows_in_order = h.in_order;
    if (to_sort == 0) return SPECK_OK;

    // the long-row temporaries (keys, two position buffers, values) and -- SUM on a view that does not start at entry 0,
    // which must come back untouched if it turns out to hold duplicates -- a copy of the view's entries
    const u32 base = h.base;
    const bool keep_copy = sum && base != 0;
    const u64 ge = h.global_entries;
    const size_t g4 = up256(ge * 4), gv = up256(ge * sizeof(T));
    const size_t copy_c = keep_copy ? up256(nnz * 4) : 0, copy_v = keep_copy ? up256(nnz * sizeof(T)) : 0;
    if (3 * g4 + gv + copy_c + copy_v) {
        rc = sc->var.ensure(3 * g4 + gv + copy_c + copy_v);
        if (rc != SPECK_OK) return rc;
    }
    unsigned char* vb = static_cast<unsigned char*>(sc->var.p);
    u32* saved_col = reinterpret_cast<u32*>(vb + 3 * g4 + gv);
    T* saved_val = reinterpret_cast<T*>(vb + 3 * g4 + gv + copy_c);
    if (keep_copy) {
        HIP_TRY(hipMemcpyAsync(saved_col, col + base, nnz * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(saved_val, val + base, nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
    }
    u32* rd = sum ? row_dups : nullptr;
    if (sum) HIP_TRY(hipMemsetAsync(row_dups, 0, size_t(rows) * 4, s));

    const u32 reg_rows = h.cnt[LIST_R8] + h.cnt[LIST_R16] + h.cnt[LIST_R32] + h.cnt[LIST_R64];
    if (h.cnt[LIST_R8])
        SPECK_LAUNCH((sort_reg_kernel<T, 8>), dim3(grid_of((h.cnt[LIST_R8] + 31) / 32, 16384)), dim3(256), 0, s, ro, col, val, rows,
                     lists, st, rd);
    if (h.cnt[LIST_R16])
        SPECK_LAUNCH((sort_reg_kernel<T, 16>), dim3(grid_of((h.cnt[LIST_R16] + 15) / 16, 16384)), dim3(256), 0, s, ro, col, val,
                     rows, lists, st, rd);
    if (h.cnt[LIST_R32])
        SPECK_LAUNCH((sort_reg_kernel<T, 32>), dim3(grid_of((h.cnt[LIST_R32] + 7) / 8, 16384)), dim3(256), 0, s, ro, col, val, rows,
                     lists, st, rd);
    if (h.cnt[LIST_R64])
        SPECK_LAUNCH((sort_reg_kernel<T, 64>), dim3(grid_of((h.cnt[LIST_R64] + 3) / 4, 16384)), dim3(256), 0, s, ro, col, val, rows,
                     lists, st, rd);
    // (the register kernels may hand rows on: the LDS launch is sized for all of them and reads the list length there)
    if (h.cnt[LIST_LDS] + reg_rows)
        SPECK_LAUNCH(sort_lds_kernel<T>, dim3(grid_of(u64(h.cnt[LIST_LDS]) + reg_rows, 8192)), dim3(256), 0, s, ro, col, val, rows,
                     lists, st, rd);
    if (h.cnt[LIST_GLOBAL]) {
        unsigned end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < (cols ? cols : 1)) ++end_bit;
        SPECK_LAUNCH(sort_global_kernel<T>, dim3(grid_of(h.cnt[LIST_GLOBAL], 2048)), dim3(256), 0, s, ro, col, val, rows, lists, st,
                     rd, reinterpret_cast<u32*>(vb), reinterpret_cast<u32*>(vb + g4), reinterpret_cast<u32*>(vb + 2 * g4),
                     reinterpret_cast<T*>(vb + 3 * g4), ge, (u32)end_bit);
    }
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->rows_sorted[0] = reg_rows - h.deferred;
        info->rows_sorted[1] = h.cnt[LIST_LDS];
        info->rows_sorted[2] = h.cnt[LIST_GLOBAL];
        info->duplicates = h.dups;
    }
    if (!sum || h.dups == 0) return SPECK_OK;
    if (keep_copy) {  // refused: the view goes back to what it was
        HIP_TRY(hipMemcpyAsync(col + base, saved_col, nnz * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(val + base, saved_val, nnz * sizeof(T), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return SPECK_ERR_INVALID;
    }

    // compaction: block sums | new row offsets | new columns | new values (the long-row temporaries are done with)
    const u64 nnz_out = nnz - h.dups;
    const u32 nblk = (rows + 1023) / 1024;
    const size_t b_sums = up256(size_t(nblk) * 4), b_ro = up256((size_t(rows) + 1) * 4), b_col = up256(nnz_out * 4);
    rc = sc->var.ensure(b_sums + b_ro + b_col + up256(nnz_out * sizeof(T)));
    if (rc != SPECK_OK) return rc;
    vb = static_cast<unsigned char*>(sc->var.p);
    u32* block_sums = reinterpret_cast<u32*>(vb);
    u32* new_ro = reinterpret_cast<u32*>(vb + b_sums);
    u32* out_col = reinterpret_cast<u32*>(vb + b_sums + b_ro);
    T* out_val = reinterpret_cast<T*>(vb + b_sums + b_ro + b_col);
    launch_exclusive_scan(s, SortNewLen{ro, row_dups}, rows, block_sums, new_ro, nullptr);
    SPECK_LAUNCH(sort_compact_kernel<T>, dim3(grid_of((u64(rows) + 3) / 4, 16384)), dim3(256), 0, s, ro, col, val, new_ro, rows,
                 out_col, out_val);
    HIP_TRY(hipMemcpyAsync(col, out_col, nnz_out * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(val, out_val, nnz_out * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ro, new_ro, (size_t(rows) + 1) * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (take_launch_error()) return SPECK_ERR_HIP;
    M->nnz = nnz_out;
    if (info) info->nnz_out = nnz_out;
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"sort lists", "sort temporaries", "M.data", "M.col_ids", "M.row_offsets"};

template <typename T>
int sort_rows_impl(speck_config* cfg, speck_dcsr* M, int flags, speck_sort_info* info)
{
    if (!M || (flags != SPECK_SORT_KEEP_DUPLICATES && flags != SPECK_SORT_SUM_DUPLICATES)) return SPECK_ERR_INVALID;
    if (M->rows > (1ull << 27) || M->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (M->nnz >= (1ull << 32)) return SPECK_ERR_INVALID;
    if ((M->rows && !M->row_offsets) || (M->nnz && (!M->col_ids || !M->data))) return SPECK_ERR_INVALID;
    if (info) {
        *info = speck_sort_info{};
        info->nnz_out = M->nnz;
    }
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (M->rows == 0) return SPECK_OK;
    SortScratch own;
    SortScratch* sc = cfg ? sort_scratch(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    int rc = sort_rows_run<T>(sc, s, M, flags, info);
    rc = check_side_guards(sc, s, M, kGuardNames, " by the row sort", rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    return rc;
}

}  // namespace

extern "C" {

int speck_sort_rows_f64(speck_config* cfg, speck_dcsr* M, int flags, speck_sort_info* info)
{
    return sort_rows_impl<double>(cfg, M, flags, info);
}

int speck_sort_rows_f32(speck_config* cfg, speck_dcsr* M, int flags, speck_sort_info* info)
{
    return sort_rows_impl<float>(cfg, M, flags, info);
}

}  // extern "C"
