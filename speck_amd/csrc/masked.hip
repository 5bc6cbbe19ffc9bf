// masked.hip -- speck_multiply_masked_*: C = M o (A B), the product kept only where the mask M has an entry.  The
// reference has no counterpart.  The table a row accumulates in IS its mask row: its size is known before a product is
// formed, it is sorted already, and a product's column is looked up with reads -- nothing is inserted, nothing is sorted.
//
//   masked_classify_kernel   one streaming pass over the rows: the input check of A and M (the offset check and the
//                            mask's rows: row_tiles.hpp; ids of A < rows(B) -- no offset or id is used as an address
//                            before it was checked), the products of the rows with work, and
//                            those rows appended to one of seven lists by mask-row length (cursors aggregated per
//                            workgroup).  B is checked by the multiply's own validate_b_kernel (stages.hip), behind it
//                            on the same stream.
//   masked_group_kernel<L>   mask rows of <= 4 L entries, L = 8 / 16 / 32 / 64 lanes per row: the mask row's columns and one
//                            double per entry in the group's slice of LDS, binary search, ds_add_f64.
//   masked_lds_kernel        a workgroup per row of <= 1024 (256 threads) or <= SPECK_MASK_LDS_MAX (1024 threads) entries:
//                            an open-addressed table of 16-bit positions over the row's columns, built once, probed read-only.
//   masked_global_kernel     a workgroup per longer row: binary search in the mask row where it lies, global atomic adds.
//   (all three walk a row's products flattened, a batch of entries of A at a time: "the product walk" below)
//   finish                   STRUCTURE: hits per row -> the shared scan (scan.hpp) -> the new row offsets; finish_subset
//                            (compact.hpp): the same scan over the hit bytes -> one streaming compaction.  FULL_PATTERN: the accumulators
//                            are C's values (fp64: accumulated in place), offsets rebased, column ids copied.
// A hit is marked in bit 31 of the column's LDS copy (columns are < 2^27).  As in the multiply a product is rounded to T,
// the sum is kept in double and rounded once.  Every kernel but the classifying pass starts after the host has read the
// verdict on all three inputs; nothing of C is written before that.
// The host side is the side operations' own (side_call.hpp: scratch, status, the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "compact.hpp"
#include "launch.hpp"
#include "masked.hpp"
#include "masked_rules.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "side_call.hpp"

using namespace speck;

namespace speck {
void MaskedScratch::release()
{
    fixed.release(), var.release();
    for (int i = 0; i < 3; ++i) {
        if (side[i]) (void)hipStreamDestroy(side[i]);
        if (join[i]) (void)hipEventDestroy(join[i]);
        side[i] = nullptr, join[i] = nullptr;
    }
    if (fork) (void)hipEventDestroy(fork);
    fork = nullptr;
}
}  // namespace speck

namespace {

// (the lists, the class limits and every rule that picks a list, a table size or a walk: masked_rules.hpp)
constexpr u32 kLdsSmall = kMaskLdsSmall, kLdsMax = kMaskLdsMax;
constexpr u32 kHitBit = 0x80000000u, kColMask = 0x7FFFFFFFu;

struct MaskedStatus {
    u32 invalid;            // offsets of A / M, an id of A
    u32 unsorted;           // a mask row
    u32 verdict_b;          // bit 2: validate_b_kernel found B wanting
    u32 idle;               // rows without work
    u32 cnt[MASK_LISTS];    // list lengths
    u32 base_m;             // M.row_offsets[0]
    u32 too_many;           // a row with work holds 2^32 products or more (the walk numbers a row's products in 32 bits)
    unsigned long long products, hits, nnz_out;
};

// (the seven lists share four regions of `rows` words: two_sided_at, device_common.hpp)

template <typename T>
struct MaskedArgs {
    const u32 *a_ro, *a_col;
    const T* a_val;
    const u32 *b_ro, *b_col;
    const T* b_val;
    const u32 *m_ro, *m_col;
    u32 rows, base_m;
    u32* lists;
    MaskedStatus* st;
    double* acc;    // one per mask entry (entry e of M's buffers at e - base_m), zero before the walk
    u8* hit;        // ... and one byte: a product fell there (nullptr: FULL_PATTERN, nobody asks)
    u32* row_cnt;   // entries hit per row, zero before the walk (nullptr: FULL_PATTERN)
};

// ------------------------------------------------------------------------------------------------ check + classify

// TILE rows and TILE threads per workgroup: 1024 where rows are short, 256 where a row holds 16 entries or more on
// average (a tile should hold enough entries to pay for its barriers, and there should be enough tiles for the machine:
// the 62 k rows of the cant stand-in are 61 tiles of 1024).  The cursors of the lists, the idle rows and the products are counted in LDS
// first and reach the status block with ONE atomic per workgroup and counter: atomics of every wave on the same few words
// of global memory cost ~8 ns each, one after the other (measured: 0.42 ms for the 1 M rows of the webbase stand-in).
template <u32 kTileRows>
__global__ __launch_bounds__(kTileRows) void masked_classify_kernel(const u32* __restrict__ a_ro, const u32* __restrict__ a_col,
                                                                    u64 a_nnz, const u32* __restrict__ b_ro, u32 b_rows, u32 b_cols,
                                                                    u64 b_nnz, const u32* __restrict__ m_ro,
                                                                    const u32* __restrict__ m_col, u64 m_nnz, u32 rows, u32 group_max,
                                                                    u32 lds_max, u32* __restrict__ lists, MaskedStatus* __restrict__ st)
{
    SPECK_POISON();
    __shared__ u32 s_aro[kTileRows + 1];
    __shared__ u32 s_mro[kTileRows + 1];
    __shared__ u32 s_bad;
    __shared__ u32 s_cnt[MASK_LISTS + 1];   // rows of the tile per list; [MASK_LISTS]: idle rows
    __shared__ u32 s_first[MASK_LISTS];     // where the tile's rows start in each list
    __shared__ unsigned long long s_products;
    __shared__ u32 s_ops[kTileRows];        // products per row (saturating well below 2^32: it only picks a group width)
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kTileRows;
    const u32 nr = min(kTileRows, rows - r0);
    const u32 base_a = a_ro[0], base_m = m_ro[0];
    if (t == 0) s_bad = 0, s_products = 0;
    if (t <= MASK_LISTS) s_cnt[t] = 0;
    s_ops[t] = 0;
    if (t == 0 && blockIdx.x == 0) st->base_m = base_m;
    __syncthreads();
    tile_offsets_load<kTileRows>(a_ro, r0, nr, base_a, a_nnz, s_aro, &s_bad);
    tile_offsets_load<kTileRows>(m_ro, r0, nr, base_m, m_nnz, s_mro, &s_bad);
    __syncthreads();
    if (tile_offsets_descend(s_aro, nr) || tile_offsets_descend(s_mro, nr)) s_bad = 1;
    __syncthreads();
    if (s_bad) {  // (nothing of col_ids is addressed through such offsets)
        if (t == 0) st->invalid = 1;
        return;
    }
    const bool unsorted = !rows_ascending_below<kTileRows>(m_col, s_mro, nr, b_cols);
    // the tile's entries of A: below rows(B); the products they stand for, where their row has a mask row
    bool bad_a = false;
    u64 products = 0;
    {
        const u64 lo = s_aro[0], hi = s_aro[nr];
#pragma unroll 4
        for (u64 i = lo + t; i < hi; i += kTileRows) {
            const u32 k = a_col[i];
            if (k >= b_rows) {
                bad_a = true;
                continue;
            }
            const u32 b0 = b_ro[k], b1 = b_ro[k + 1];
            const u64 len = b1 > b0 ? min(u64(b1 - b0), b_nnz) : 0ull;  // (B's own check speaks later: clamped)
            const u32 r = first_end_beyond(s_aro + 1, nr, i);  // the row of entry i
            if (s_mro[r + 1] > s_mro[r]) {
                products += len;
                if (s_ops[r] < kMaskOpsCeiling) atomicAdd(&s_ops[r], (u32)min(len, u64(kMaskOpsAddCap)));
            }
        }
    }
    __syncthreads();
    if (unsorted) st->unsorted = 1;
    if (bad_a) st->invalid = 1;
    const u32 lane = lane_id();
    wave_counter_to_lds(&s_products, products);
    int cls = -2;  // no row
    if (t < nr) {
        const u32 len = s_mro[t + 1] - s_mro[t];
        if (len == 0 || s_aro[t + 1] == s_aro[t]) cls = MASK_LISTS;
        else cls = (int)mask_list_of(len, s_ops[t], group_max, lds_max);
    }
    u32 rank = 0;  // of my row among the tile's rows of its list
#pragma unroll
    for (int k = 0; k <= MASK_LISTS; ++k) {
        const u64 m = __ballot(cls == k);
        if (m == 0) continue;
        const u32 leader = (u32)__ffsll((long long)m) - 1u;
        u32 first = 0;
        if (lane == leader) first = atomicAdd(&s_cnt[k], (u32)__popcll(m));
        first = (u32)__shfl((int)first, (int)leader);
        if (cls == k) rank = first + (u32)__popcll(m & lanemask_lt());
    }
    __syncthreads();
    if ((s_products >> 32) != 0 && cls >= 0 && cls < MASK_LISTS) {  // (never on a real input: a thread sums its own row)
        u64 ops = 0;
        for (u32 i = s_aro[t]; i < s_aro[t + 1]; ++i) {
            const u32 k = a_col[i];
            if (k >= b_rows) continue;
            const u32 b0 = b_ro[k], b1 = b_ro[k + 1];
            ops += b1 > b0 ? min(u64(b1 - b0), b_nnz) : 0ull;
        }
        if ((ops >> 32) != 0) st->too_many = 1;
    }
    if (t < MASK_LISTS && s_cnt[t]) s_first[t] = atomicAdd(&st->cnt[t], s_cnt[t]);
    if (t == MASK_LISTS && s_cnt[t]) atomicAdd(&st->idle, s_cnt[t]);
    lds_counter_to_status(&st->products, &s_products, MASK_LISTS + 1u);
    __syncthreads();
    if (cls >= 0 && cls < MASK_LISTS) *two_sided_at(lists, rows, (u32)cls, s_first[cls] + rank) = r0 + t;
}

// ------------------------------------------------------------------------------------------------ the product walk
// All three classes walk a row's products FLATTENED, a batch of entries of A at a time: every lane of the group takes one
// entry of the batch (its column, the bounds of "its" row of B), an inclusive scan of the B-row lengths numbers the
// batch's products, and the lanes stride over those numbers -- a product's entry of A is found by binary search over
// the scan (LDS).  The chain of dependent loads (A.col -> B.row_offsets -> B.col) is paid once per batch, not once per
// entry of A, and no lane idles on a short row of B.  (First form: teams of eight lanes per entry of A, one entry after
// the other -- a row of 256 entries of A cost 32 such chains, 120 us for a handful of rows of the scircuit stand-in.)
// `end[i]`: products of the batch up to and including entry i;  `off[i]`: first entry of its B row - products before it.
// The walk itself is walk_products (row_tiles.hpp); each class brings its `apply`: how a product's column is looked up in
// the mask row, and where a hit is added.  The hits of a workgroup reach the status block with one atomic (block_counter_to).

// ------------------------------------------------------------------------------------------------ group class
// 256 threads = 256 / L groups; per group 4 L columns and 4 L doubles of LDS for the mask row, 2 L words and L values for
// the batch (16 KiB per workgroup whatever L): eight workgroups per CU, bounded by waves.
template <typename T, u32 L>
__global__ __launch_bounds__(256) void masked_group_kernel(const MaskedArgs<T> g)
{
    SPECK_POISON();
    constexpr u32 NG = 256 / L, NP = 4 * L;
    constexpr u32 K = L == 8 ? LIST_G8 : L == 16 ? LIST_G16 : L == 32 ? LIST_G32 : LIST_G64;
    __shared__ double s_acc[NG * NP];
    __shared__ u32 s_col[NG * NP];
    __shared__ u32 s_end[256], s_off[256];
    __shared__ T s_av[256];
    __shared__ unsigned long long s_hits;
    const u32 wl = lane_id(), gl = wl & (L - 1u), base_lane = wl & ~(L - 1u);
    const u32 gid = threadIdx.x / L;
    double* acc = s_acc + gid * NP;
    u32* col = s_col + gid * NP;
    u32* end = s_end + gid * L;
    u32* off = s_off + gid * L;
    T* av = s_av + gid * L;
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    const u32 n_list = g.st->cnt[K];
    u64 hits = 0;
    for (u32 e = blockIdx.x * NG + gid; e < n_list; e += gridDim.x * NG) {
        const u32 row = *two_sided_at(g.lists, g.rows, K, e);
        const u32 m0 = g.m_ro[row], n = min(g.m_ro[row + 1] - m0, NP);
        const u32 a0 = g.a_ro[row], a1 = g.a_ro[row + 1];
#pragma unroll
        for (u32 u = 0; u < 4; ++u) {
            const u32 p = u * L + gl;
            if (p < n) {
                col[p] = g.m_col[m0 + p];
                acc[p] = 0.0;
            }
        }
        wave_lds_fence();
        const u32 cmin = col[0], cmax = col[n - 1];  // (n >= 1: a row with work; no hit is marked yet)
        // (ab in 64 bits: a view may end at entry 2^32 - 1, and a u32 `ab += L` past it starts over at 0)
        for (u64 ab = a0; ab < a1; ab += L) {
            const u32 nb = min(L, (u32)(a1 - ab));
            u32 len = 0, b0 = 0;
            if (gl < nb) {
                const u32 k = g.a_col[ab + gl];
                av[gl] = g.a_val[ab + gl];
                b0 = g.b_ro[k];
                len = g.b_ro[k + 1] - b0;
            }
            u32 incl = len;
#pragma unroll
            for (u32 d = 1; d < L; d <<= 1) {
                const u32 up = (u32)__shfl_up((int)incl, d, (int)L);
                if (gl >= d) incl += up;
            }
            const u32 total = (u32)__shfl((int)incl, (int)(L - 1u), (int)L);
            end[gl] = incl;
            off[gl] = b0 - (incl - len);
            wave_lds_fence();
            // a product whose column `c` of B is in a register: looked up in the mask row, added on a hit
            // (the four searches of a lane in lockstep, branch-free, lost: the products outside the mask row's span pay
            //  for a search then -- cant stand-in 1.24 -> 1.47 ms, webbase triangles 0.74 -> 0.91 ms)
            auto apply = [&](u32 i, u32 j, u32 c) {
                if (c < cmin || c > cmax) return;
                // (not lower_bound_in_row: the words searched are LDS copies that carry the hit bit)
                u32 lo = 0, hi = n;
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if ((col[mid] & kColMask) < c) lo = mid + 1; else hi = mid;
                }
                if (lo >= n) return;
                const u32 v = col[lo];
                if ((v & kColMask) != c) return;
                const T prod = av[i] * g.b_val[j];
                atomicAdd(&acc[lo], (double)prod);
                if (!(v & kHitBit)) atomicOr(&col[lo], kHitBit);
                ++hits;
            };
            // (four loads of B's columns in flight per lane in either walk: a walk is a chain of such loads otherwise)
            if (mask_team_walk(total, nb)) {
                // long rows of B (16 entries on average): teams of eight lanes take the batch's entries in turn and walk
                // "their" row eight entries at a time -- no search for the entry of A
                constexpr u32 NT = L / 8u;
                for (u32 i = gl / 8u; i < nb; i += NT) {
                    const u32 before = i ? end[i - 1] : 0u;
                    const u32 j1 = off[i] + end[i];
                    for (u32 j = off[i] + before + (gl & 7u); j < j1; j += 4u * 8u) {
                        u32 c[4];
#pragma unroll
                        for (u32 u = 0; u < 4; ++u) c[u] = j + u * 8u < j1 ? g.b_col[j + u * 8u] : kNoColumn;
#pragma unroll
                        for (u32 u = 0; u < 4; ++u) apply(i, j + u * 8u, c[u]);
                    }
                }
            } else walk_products<L>(gl, end, off, nb, total, g.b_col, apply);
            wave_lds_fence();  // the next batch overwrites end / off
        }
        u32 cnt = 0;
#pragma unroll
        for (u32 u = 0; u < 4; ++u) {
            const u32 p = u * L + gl;
            const bool h = p < n && (col[p] & kHitBit);
            if (h) {
                const size_t at = size_t(m0 - g.base_m) + p;
                g.acc[at] = acc[p];
                if (g.hit) g.hit[at] = 1;
            }
            const u64 m = __ballot(h);
            cnt += (u32)__popcll(L == 64 ? m : (m >> base_lane) & ((1ull << (L & 63u)) - 1ull));
        }
        if (gl == 0 && g.row_cnt) g.row_cnt[row] = cnt;
        wave_lds_fence();  // the next row overwrites the slice
    }
    block_counter_to(&g.st->hits, hits, &s_hits);
}

// ------------------------------------------------------------------------------------------------ LDS class
// One workgroup per row.  Dynamic LDS for `cap` entries: cap doubles | cap columns | 2 cap table slots of 16 bits, each the
// position of a column in the row or 0xFFFF | 2 THREADS words for the batch.  cap = 1024, 256 threads: 18 KiB, eight
// workgroups per CU by waves; cap = 4096, 1024 threads: 72 KiB, two workgroups per CU.  A row's table is the smallest
// power of two >= twice its length (load <= 1/2): clearing and building cost what the row is long, not what the class
// admits.  The columns of a row are distinct, so building the table races only for empty slots: one compare-and-swap on
// the word that holds the slot, repeated when the OTHER half of the word changed meanwhile.  Probes read.
// (the table's size and a column's home slot: mask_table_bits, table_slot -- masked_rules.hpp)
template <typename T, u32 THREADS>
__global__ __launch_bounds__(THREADS) void masked_lds_kernel(const MaskedArgs<T> g, u32 list, u32 cap)
{
    SPECK_POISON();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ u32 s_scan[THREADS / 64 + 1];
    __shared__ unsigned long long s_hits;
    double* acc = reinterpret_cast<double*>(smem);
    u32* col = reinterpret_cast<u32*>(smem + size_t(cap) * 8);
    u32* tab = col + cap;
    u32* end = tab + cap;
    u32* off = end + THREADS;
    const u32 t = threadIdx.x;
    if (t == 0) s_hits = 0;
    const u32 n_list = g.st->cnt[list];
    u64 hits = 0;
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(g.lists, g.rows, list, e);
        const u32 m0 = g.m_ro[row], n = min(g.m_ro[row + 1] - m0, cap);
        const u32 a0 = g.a_ro[row], a1 = g.a_ro[row + 1];
        const u32 bits = mask_table_bits(n);
        const u32 slots = 1u << bits;
        for (u32 p = t; p < n; p += THREADS) {
            col[p] = g.m_col[m0 + p];
            acc[p] = 0.0;
        }
        for (u32 w = t; w < slots / 2; w += THREADS) tab[w] = 0xFFFFFFFFu;
        __syncthreads();
        for (u32 p = t; p < n; p += THREADS) {
            u32 s = table_slot(col[p], bits);
            while (true) {
                u32* w = &tab[s >> 1];
                const u32 sh = (s & 1u) * 16u;
                const u32 old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (((old >> sh) & 0xFFFFu) != 0xFFFFu) {
                    s = (s + 1u) & (slots - 1u);
                    continue;
                }
                if (atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (p << sh)) == old) break;
            }
        }
        const u32 cmin = col[0], cmax = col[n - 1];  // (no hit is marked before the barriers of the first batch)
        for (u64 ab = a0; ab < a1; ab += THREADS) {  // (64 bits: as in the group class)
            const u32 nb = min(THREADS, (u32)(a1 - ab));
            u32 len = 0, b0 = 0;
            if (t < nb) {
                const u32 k = g.a_col[ab + t];
                b0 = g.b_ro[k];
                len = g.b_ro[k + 1] - b0;
            }
            u32 total;
            const u32 excl = block_exclusive_scan<THREADS>(len, s_scan, &total);  // (its barriers: the table is built)
            end[t] = excl + len;
            off[t] = b0 - excl;
            __syncthreads();
            auto apply = [&](u32 i, u32 j, u32 c) {
                if (c < cmin || c > cmax) return;  // (rows of B ascend: only the part inside the mask row's span can hit)
                u32 s = table_slot(c, bits);
                while (true) {
                    const u32 q = (tab[s >> 1] >> ((s & 1u) * 16u)) & 0xFFFFu;
                    if (q == 0xFFFFu) return;
                    const u32 v = col[q];
                    if ((v & kColMask) == c) {
                        const T prod = g.a_val[ab + i] * g.b_val[j];
                        atomicAdd(&acc[q], (double)prod);
                        if (!(v & kHitBit)) atomicOr(&col[q], kHitBit);
                        ++hits;
                        return;
                    }
                    s = (s + 1u) & (slots - 1u);
                }
            };
            walk_products<THREADS>(t, end, off, nb, total, g.b_col, apply);
            __syncthreads();  // the next batch overwrites end / off
        }
        u32 cnt = 0;
        for (u32 p = t; p < n; p += THREADS)
            if (col[p] & kHitBit) {
                const size_t at = size_t(m0 - g.base_m) + p;
                g.acc[at] = acc[p];
                if (g.hit) g.hit[at] = 1;
                ++cnt;
            }
        if (g.row_cnt) {
            cnt = wave_reduce_add(cnt);
            if (lane_id() == 0 && cnt) atomicAdd(&g.row_cnt[row], cnt);
        }
        __syncthreads();  // the next row overwrites the table
    }
    __syncthreads();
    block_counter_to(&g.st->hits, hits, &s_hits);
}

// ------------------------------------------------------------------------------------------------ global class
// One workgroup per row; the mask row is searched where it lies, a product is added to its accumulator with a global
// atomic, the hit byte is a plain store of 1 (every writer stores the same).  Serves a handful of rows: correct first.
template <typename T>
__global__ __launch_bounds__(1024) void masked_global_kernel(const MaskedArgs<T> g)
{
    SPECK_POISON();
    constexpr u32 THREADS = 1024;
    __shared__ u32 s_end[THREADS], s_off[THREADS];
    __shared__ u32 s_scan[THREADS / 64 + 1];
    __shared__ unsigned long long s_hits;
    const u32 t = threadIdx.x;
    if (t == 0) s_hits = 0;
    const u32 n_list = g.st->cnt[LIST_GLOBAL];
    u64 hits = 0;
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(g.lists, g.rows, LIST_GLOBAL, e);
        const u32 m0 = g.m_ro[row], n = g.m_ro[row + 1] - m0;
        const u32 a0 = g.a_ro[row], a1 = g.a_ro[row + 1];
        const u32* mc = g.m_col + m0;
        const size_t at0 = size_t(m0 - g.base_m);
        const u32 cmin = mc[0], cmax = mc[n - 1];
        for (u64 ab = a0; ab < a1; ab += THREADS) {  // (64 bits: as in the group class)
            const u32 nb = min(THREADS, (u32)(a1 - ab));
            u32 len = 0, b0 = 0;
            if (t < nb) {
                const u32 k = g.a_col[ab + t];
                b0 = g.b_ro[k];
                len = g.b_ro[k + 1] - b0;
            }
            u32 total;
            const u32 excl = block_exclusive_scan<THREADS>(len, s_scan, &total);
            s_end[t] = excl + len;
            s_off[t] = b0 - excl;
            __syncthreads();
            auto apply = [&](u32 i, u32 j, u32 c) {
                if (c < cmin || c > cmax) return;
                const u32 lo = lower_bound_in_row(mc, 0u, n, c);
                if (lo >= n || mc[lo] != c) return;
                const T prod = g.a_val[ab + i] * g.b_val[j];
                atomicAdd(&g.acc[at0 + lo], (double)prod);
                if (g.hit) g.hit[at0 + lo] = 1;
                ++hits;
            };
            walk_products<THREADS>(t, s_end, s_off, nb, total, g.b_col, apply);
            __syncthreads();  // the next batch overwrites end / off
        }
        if (g.row_cnt) {
            __threadfence_block();
            __syncthreads();  // the row's hit bytes are complete
            u32 cnt = 0;
            for (u32 p = t; p < n; p += THREADS) cnt += g.hit[at0 + p] ? 1u : 0u;
            cnt = wave_reduce_add(cnt);
            if (lane_id() == 0 && cnt) atomicAdd(&g.row_cnt[row], cnt);
        }
    }
    __syncthreads();
    block_counter_to(&g.st->hits, hits, &s_hits);
}

// ------------------------------------------------------------------------------------------------ finish
// STRUCTURE: hits per row -> the shared exclusive scan (scan.hpp): the new row offsets, nnz(C) into the status block.  C's
// entries are M's entries with a hit, in M's order: finish_subset (compact.hpp), from the accumulators (double) to T.

// FULL_PATTERN: C.row_offsets = M.row_offsets rebased to 0; the values rounded where the accumulators are not C's own
__global__ __launch_bounds__(256) void masked_rebase_kernel(const u32* __restrict__ m_ro, u32 rows, u32* __restrict__ c_ro)
{
    SPECK_POISON();
    const u32 base = m_ro[0];
    for (u64 r = u64(blockIdx.x) * 256 + threadIdx.x; r <= rows; r += u64(gridDim.x) * 256) c_ro[r] = m_ro[r] - base;
}

template <typename T>
__global__ __launch_bounds__(256) void masked_round_kernel(const double* __restrict__ acc, u64 n, T* __restrict__ out)
{
    SPECK_POISON();
    for (u64 i = u64(blockIdx.x) * 256 + threadIdx.x; i < n; i += u64(gridDim.x) * 256) out[i] = (T)acc[i];
}

// ------------------------------------------------------------------------------------------------ host
// dynamic LDS of the LDS class: accumulators | columns | table | batch
constexpr u32 lds_bytes(u32 cap, u32 threads) { return cap * 16u + threads * 8u; }

template <typename T>
int masked_run(MaskedScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* M, speck_dcsr* C,
               bool full, speck_masked_info* info, COut* out)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz_m = M->nnz;
    if (rows == 0) return publish_empty_c(C, B->cols, sizeof(T), s, out);

    // status | lists (four regions of `rows` words) | hits per row | new row offsets | workgroup sums of the scan
    RowScratch<MaskedStatus> f;
    int rc = carve_row_scratch(&sc->fixed, rows, size_t(4) * rows, &f);
    if (rc != SPECK_OK) return rc;
    MaskedStatus* st = f.st;
    u32 *lists = f.lists, *row_cnt = f.row_cnt;
    // accumulators | hit bytes | hits per tile of the compaction
    const bool acc_in_c = full && std::is_same<T, double>::value;
    const u32 ntiles = (u32)((nnz_m + kCompactTile - 1) / kCompactTile);
    const size_t acc_bytes = acc_in_c ? 0 : up256(nnz_m * 8), hit_bytes = full ? 0 : up256(nnz_m);
    const size_t tile_bytes = full ? 0 : up256(size_t(ntiles) * 4);
    if (acc_bytes + hit_bytes + tile_bytes) {
        rc = sc->var.ensure(acc_bytes + hit_bytes + tile_bytes);
        if (rc != SPECK_OK) return rc;
    }
    unsigned char* vb = static_cast<unsigned char*>(sc->var.p);

    // ---- the verdict on A, M (this file) and B (the multiply's check), read before anything else starts
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(MaskedStatus), s));
    constexpr u32 kTL = kMaskTileRowsLong, kTS = kMaskTileRowsShort;  // (below: the tile of long rows, of short rows)
    if ((A->nnz + nnz_m) / rows >= kMaskLongRowAvg)
        SPECK_LAUNCH(masked_classify_kernel<kTL>, dim3((rows + kTL - 1) / kTL), dim3(kTL), 0, s, A->row_offsets, A->col_ids, A->nnz,
                     B->row_offsets, (u32)B->rows, (u32)B->cols, B->nnz, M->row_offsets, M->col_ids, nnz_m, rows, sc->group_max,
                     sc->lds_max, lists, st);
    else
        SPECK_LAUNCH(masked_classify_kernel<kTS>, dim3((rows + kTS - 1) / kTS), dim3(kTS), 0, s, A->row_offsets, A->col_ids, A->nnz,
                     B->row_offsets, (u32)B->rows, (u32)B->cols, B->nnz, M->row_offsets, M->col_ids, nnz_m, rows, sc->group_max,
                     sc->lds_max, lists, st);
    launch_validate_b(s, B->row_offsets, B->col_ids, (u32)B->rows, (u32)B->cols, B->nnz, &st->verdict_b);
    MaskedStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    if (h.unsorted || (h.verdict_b & 4u)) return SPECK_ERR_UNSORTED;
    if (h.too_many) return SPECK_ERR_DIM_LIMIT;

    // ---- one product walk per row with work
    if (full) {
        rc = prepare_c(C, rows, nnz_m, sizeof(T), out);
        if (rc != SPECK_OK) return rc;
    }
    double* acc = acc_in_c ? static_cast<double*>(out->val) : reinterpret_cast<double*>(vb);
    u8* hit = full ? nullptr : vb + acc_bytes;
    if (nnz_m) {
        HIP_TRY(hipMemsetAsync(acc, 0, nnz_m * 8, s));
        if (hit) HIP_TRY(hipMemsetAsync(hit, 0, nnz_m, s));
    }
    if (!full) HIP_TRY(hipMemsetAsync(row_cnt, 0, (size_t(rows) + 1) * 4, s));
    const MaskedArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), B->row_offsets, B->col_ids,
                          static_cast<const T*>(B->data), M->row_offsets, M->col_ids, rows, h.base_m, lists, st, acc, hit,
                          full ? nullptr : row_cnt};
    // (grids: what a CU keeps resident x 256 CUs at most -- the kernels stride over their lists)
    // The classes hold disjoint rows and are bound by latency more than by throughput (a launch lasts as long as its
    // heaviest rows): the narrow groups stay on the call's stream, the others run beside them on side streams.
    const bool work[4] = {h.cnt[LIST_G8] != 0, (h.cnt[LIST_G16] | h.cnt[LIST_G32]) != 0, h.cnt[LIST_G64] != 0,
                          (h.cnt[LIST_LDS_S] | h.cnt[LIST_LDS_L] | h.cnt[LIST_GLOBAL]) != 0};
    const bool forked = work[0] + work[1] + work[2] + work[3] >= 2;
    hipStream_t on[4] = {s, s, s, s};
    if (forked) {
        if (!sc->fork) {
            HIP_TRY(hipEventCreateWithFlags(&sc->fork, hipEventDisableTiming));
            for (int i = 0; i < 3; ++i) {
                HIP_TRY(hipStreamCreateWithFlags(&sc->side[i], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&sc->join[i], hipEventDisableTiming));
            }
        }
        HIP_TRY(hipEventRecord(sc->fork, s));
        for (int i = 1; i < 4; ++i)
            if (work[i]) {
                on[i] = sc->side[i - 1];
                HIP_TRY(hipStreamWaitEvent(on[i], sc->fork, 0));
            }
    }
    if (h.cnt[LIST_G8]) SPECK_LAUNCH((masked_group_kernel<T, 8>), dim3(grid_of((h.cnt[LIST_G8] + 31) / 32, 2048)), dim3(256), 0, on[0], g);
    if (h.cnt[LIST_G16]) SPECK_LAUNCH((masked_group_kernel<T, 16>), dim3(grid_of((h.cnt[LIST_G16] + 15) / 16, 2048)), dim3(256), 0, on[1], g);
    if (h.cnt[LIST_G32]) SPECK_LAUNCH((masked_group_kernel<T, 32>), dim3(grid_of((h.cnt[LIST_G32] + 7) / 8, 2048)), dim3(256), 0, on[1], g);
    if (h.cnt[LIST_G64]) SPECK_LAUNCH((masked_group_kernel<T, 64>), dim3(grid_of((h.cnt[LIST_G64] + 3) / 4, 2048)), dim3(256), 0, on[2], g);
    if (h.cnt[LIST_LDS_S])
        SPECK_LAUNCH((masked_lds_kernel<T, 256>), dim3(grid_of(h.cnt[LIST_LDS_S], 2048)), dim3(256), lds_bytes(kLdsSmall, 256), on[3], g,
                     (u32)LIST_LDS_S, kLdsSmall);
    if (h.cnt[LIST_LDS_L]) {
        // more than 64 KiB of LDS needs the opt-in (with every launch, as numeric.hip does: it belongs to the current device)
        note_launch_status(hipFuncSetAttribute(reinterpret_cast<const void*>(&masked_lds_kernel<T, 1024>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kLdsMax, 1024)),
                           "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        SPECK_LAUNCH((masked_lds_kernel<T, 1024>), dim3(grid_of(h.cnt[LIST_LDS_L], 512)), dim3(1024), lds_bytes(kLdsMax, 1024), on[3], g,
                     (u32)LIST_LDS_L, kLdsMax);
    }
    if (h.cnt[LIST_GLOBAL]) SPECK_LAUNCH(masked_global_kernel<T>, dim3(grid_of(h.cnt[LIST_GLOBAL], 512)), dim3(1024), 0, on[3], g);
    if (forked)
        for (int i = 1; i < 4; ++i)
            if (work[i]) {
                HIP_TRY(hipEventRecord(sc->join[i - 1], on[i]));
                HIP_TRY(hipStreamWaitEvent(s, sc->join[i - 1], 0));
            }

    // ---- finish
    u64 nnz_out = nnz_m;
    if (!full) launch_exclusive_scan(s, CountArray{row_cnt}, rows, f.block_sums, f.new_ro, &st->nnz_out);
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (!full) {
        nnz_out = h.nnz_out;
        rc = prepare_c(C, rows, nnz_out, sizeof(T), out);
        if (rc != SPECK_OK) return rc;
        const KeepWord words{reinterpret_cast<const u32*>(hit), nnz_m};
        rc = finish_subset<double, T>(s, words, reinterpret_cast<u32*>(vb + acc_bytes + hit_bytes), M->col_ids + h.base_m, acc,
                                      f.new_ro, rows, B->cols, nnz_out, C, out);
        if (rc != SPECK_OK) return rc;
    } else {
        SPECK_LAUNCH(masked_rebase_kernel, dim3(grid_of((u64(rows) + 256) / 256, 4096)), dim3(256), 0, s, M->row_offsets, rows, out->ro);
        if (nnz_m) {
            HIP_TRY(hipMemcpyAsync(out->col, M->col_ids + h.base_m, nnz_m * 4, hipMemcpyDeviceToDevice, s));
            if (!acc_in_c)
                SPECK_LAUNCH(masked_round_kernel<T>, dim3(grid_of((nnz_m + 255) / 256, 8192)), dim3(256), 0, s, acc, nnz_m,
                             static_cast<T*>(out->val));
        }
        HIP_TRY(hipStreamSynchronize(s));
        if (take_launch_error()) return SPECK_ERR_HIP;
        publish_c(C, rows, B->cols, nnz_out, out);
    }
    if (info) {
        info->rows_idle = h.idle;
        info->rows_class[0] = u64(h.cnt[LIST_G8]) + h.cnt[LIST_G16] + h.cnt[LIST_G32] + h.cnt[LIST_G64];
        info->rows_class[1] = u64(h.cnt[LIST_LDS_S]) + h.cnt[LIST_LDS_L];
        info->rows_class[2] = h.cnt[LIST_GLOBAL];
        info->products = h.products;
        info->hits = h.hits;
        info->nnz_out = nnz_out;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"masked lists", "masked accumulators", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int masked_impl(speck_config* cfg, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* M, speck_dcsr* C, int flags,
                speck_masked_info* info)
{
    if (!A || !B || !M || !C) return SPECK_ERR_INVALID;
    if (flags != SPECK_MASK_STRUCTURE && flags != SPECK_MASK_FULL_PATTERN) return SPECK_ERR_INVALID;
    if (A->cols != B->rows || M->rows != A->rows || M->cols != B->cols) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || B->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32) || B->nnz >= (1ull << 32) || M->nnz >= (1ull << 32)) return SPECK_ERR_INVALID;
    if (!csr_args_ok(A, true) || !csr_args_ok(B, true) || !csr_args_ok(M, false)) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A) || shares_buffer(C, B) || shares_buffer(C, M)) return SPECK_ERR_INVALID;
    if (info) *info = speck_masked_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, masked_scratch, C, info, kGuardNames, " by the masked product",
                         [&](MaskedScratch* sc, hipStream_t s, COut* out) {
                             return masked_run<T>(sc, s, A, B, M, C, flags == SPECK_MASK_FULL_PATTERN, info, out);
                         });
}

}  // namespace

extern "C" {

int speck_multiply_masked_f64(speck_config* cfg, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* M, speck_dcsr* C,
                              int flags, speck_masked_info* info)
{
    return masked_impl<double>(cfg, A, B, M, C, flags, info);
}

int speck_multiply_masked_f32(speck_config* cfg, const speck_dcsr* A, const speck_dcsr* B, const speck_dcsr* M, speck_dcsr* C,
                              int flags, speck_masked_info* info)
{
    return masked_impl<float>(cfg, A, B, M, C, flags, info);
}

}  // extern "C"
