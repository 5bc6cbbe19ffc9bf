// topk.hip -- speck_topk_*: C = the k largest entries of every row of A (by value, by -value or by magnitude), in input
// order, copied bit for bit.  The reference has no counterpart.
//
//   topk_classify_kernel   one streaming pass over row_offsets and col_ids, the shape of sort_classify_kernel: the input
//                          check (the offset check: row_tiles.hpp; ids < cols -- no offset is used as an address before it
//                          was checked) and, per row, min(len, k) into row_cnt.  The shared scan (scan.hpp) turns these
//                          into C's offsets: they depend on the lengths alone -- no marking pass, no keep byte.  Rows
//                          longer than k go to one of six lists by length (wave-aggregated integer cursors).
//                          The ONE read-back in front of C: the verdict, nnz(C), the list lengths.
//   topk_copy_kernel       the rows of at most k entries: a tile of 256 rows, the entries to copy numbered through in LDS,
//                          a thread per entry, four loads in flight.  Knows nothing of keys (it counts the NaNs it copies
//                          with an integer test on the bits).  On a matrix without a longer row the call is this copy.
//   topk_group_kernel<L>   rows of <= 4 L entries, L = 8 / 16 / 32 / 64 lanes per row: the row's keys -- order-preserving
//                          unsigned integers, 64 bits for double and 32 for float -- staged in LDS; every lane counts, for
//                          its (up to) four entries, the entries that beat them (a larger key, or an equal one in front)
//                          and keeps those with fewer than k; written at the ballot prefix inside the group.
//   topk_row_kernel        one workgroup per longer row: a radix select from the most significant byte -- a histogram of
//                          256 bins in LDS per pass, a suffix scan of the bins, narrowed to the bin that holds the k-th key;
//                          it stops where the narrowed set is exactly what is still needed -- gives the threshold key tau
//                          and t, the entries to keep among the keys that equal it.  Then ONE ordered walk keeps key > tau
//                          and the first t of key == tau; an entry's place is the number of kept entries in front of it
//                          (one packed block scan per 256 / 1024 entries, the counts carried on).  kLds: 256 threads, the
//                          keys of the row (<= SPECK_TOPK_LDS_MAX) in LDS.  Otherwise 1024 threads, the values read again
//                          from global memory in every pass, four loads in flight per lane: a hub's row stays in L2 / MALL,
//                          nothing is moved, there is no temporary.
// Keys, counts and offsets are integers everywhere: no floating-point atomic and no floating-point arithmetic at all.
// The host side is the side operations' own (side_call.hpp: scratch, status, the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "compact.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "side_call.hpp"
#include "topk.hpp"

using namespace speck;

namespace {

constexpr u32 kGroupMax = SPECK_TOPK_GROUP_MAX, kLdsMax = SPECK_TOPK_LDS_MAX;
constexpr u32 kPer = 4;  // entries a lane of a group holds; loads a thread of the row kernels keeps in flight
static_assert(kGroupMax == 64 * kPer, "the widest group is a wave");
enum { LIST_G8 = 0, LIST_G16, LIST_G32, LIST_G64, LIST_LDS, LIST_LONG, TOPK_LISTS };
constexpr u32 kGroupGrid = 2048, kLdsGrid = 2048, kLongGrid = 1024, kCopyTileRows = 256;  // workgroups of a launch at most

struct TopkStatus {
    u32 invalid;           // offsets of A, an id of A
    u32 max_row;           // the longest row of C
    u32 entries;           // A.row_offsets[rows] - A.row_offsets[0] (== nnz, or the call is refused)
    u32 ties_cut;          // rows in which a dropped entry has the key of a kept one
    u32 cnt[TOPK_LISTS];   // list lengths
    unsigned long long nnz_out, nan_kept;
};

// (the six lists share three regions of `rows` words: two_sided_at, device_common.hpp)

// ------------------------------------------------------------------------------------------------ keys
// The IEEE bits after the mode's sign operation, -0.0 -> +0.0, sign-flipped the usual way: a larger key is a better
// entry.  A NaN is all ones, above +inf (0xFFF0.. / 0xFF80..) in every mode.  Integer operations only.
template <typename T>
struct KeyOf {
    using type = u64;
};
template <>
struct KeyOf<float> {
    using type = u32;
};

__device__ __forceinline__ u64 value_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ u32 value_bits(float v) { return __float_as_uint(v); }

template <typename K>
__device__ __forceinline__ K key_of_bits(K b, u32 mode)
{
    constexpr K kSign = K(1) << (sizeof(K) * 8 - 1);
    constexpr K kInf = sizeof(K) == 8 ? (K)0x7FF0000000000000ull : (K)0x7F800000u;
    const K mag = b & ~kSign;
    if (mag > kInf) return ~K(0);
    if (mode == SPECK_TOPK_SMALLEST) b ^= kSign;
    else if (mode == SPECK_TOPK_LARGEST_ABS) b = mag;
    if (b == kSign) b = 0;
    return (b & kSign) ? ~b : (b | kSign);
}

template <typename K>
__device__ __forceinline__ bool bits_are_nan(K b)
{
    constexpr K kSign = K(1) << (sizeof(K) * 8 - 1);
    constexpr K kInf = sizeof(K) == 8 ? (K)0x7FF0000000000000ull : (K)0x7F800000u;
    return (b & ~kSign) > kInf;
}

// ------------------------------------------------------------------------------------------------ check + classify
constexpr u32 kClassifyThreads = 512, kClassifyUnroll = 4;

template <u32 kTileRows>
__global__ __launch_bounds__(kClassifyThreads) void topk_classify_kernel(const u32* __restrict__ ro, const u32* __restrict__ col, u32 rows,
                                                                         u32 cols, u64 nnz, u32 k, u32 group_max, u32 lds_max,
                                                                         u32* __restrict__ row_cnt, u32* __restrict__ lists,
                                                                         TopkStatus* __restrict__ st)
{
    SPECK_POISON();
    static_assert(kTileRows <= kClassifyThreads, "a thread per row classifies");
    __shared__ u32 s_ro[kTileRows + 1];
    __shared__ u32 s_bad;
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kTileRows;
    const u32 nr = min(kTileRows, rows - r0);
    const u32 base = ro[0];
    if (t == 0) s_bad = 0;
    __syncthreads();
    tile_offsets_load<kClassifyThreads>(ro, r0, nr, base, nnz, s_ro, &s_bad);
    __syncthreads();
    if (tile_offsets_descend(s_ro, nr)) s_bad = 1;
    __syncthreads();
    if (s_bad) {  // (nothing of col_ids is addressed through such offsets)
        if (t == 0) st->invalid = 1;
        return;
    }
    if (t == 0 && r0 + nr == rows) st->entries = s_ro[nr] - base;
    // the tile's ids: offsets are monotone and inside [base, base + nnz] here
    const u64 lo = s_ro[0], hi = s_ro[nr];
    bool bad_col = false;
    for (u64 i0 = lo + t; i0 < hi; i0 += kClassifyThreads * kClassifyUnroll) {
        u32 c[kClassifyUnroll];
#pragma unroll
        for (u32 u = 0; u < kClassifyUnroll; ++u) {
            const u64 i = i0 + u * kClassifyThreads;
            c[u] = i < hi ? col[i] : 0u;
        }
#pragma unroll
        for (u32 u = 0; u < kClassifyUnroll; ++u) bad_col |= c[u] >= cols;  // (an idle slot holds 0; cols >= 1 where an entry exists)
    }
    if (bad_col) st->invalid = 1;
    int cls = -1;  // no row, or a row that is kept whole
    u32 kept = 0;
    if (t < nr) {
        const u32 len = s_ro[t + 1] - s_ro[t];
        kept = min(len, k);
        row_cnt[r0 + t] = kept;
        if (len > k) {
            if (len <= group_max && len <= kGroupMax)
                cls = len <= kGroupMax / 8 ? LIST_G8 : len <= kGroupMax / 4 ? LIST_G16 : len <= kGroupMax / 2 ? LIST_G32 : LIST_G64;
            else cls = (len <= lds_max && len <= kLdsMax) ? LIST_LDS : LIST_LONG;
        }
    }
    const u32 lane = lane_id();
    const u32 longest = wave_reduce_max(kept);
    if (lane == 0 && longest) atomicMax(&st->max_row, longest);
#pragma unroll
    for (int c = 0; c < TOPK_LISTS; ++c) {
        const u64 m = __ballot(cls == c);
        if (m == 0) continue;
        const u32 leader = (u32)__ffsll((long long)m) - 1u;
        u32 first = 0;
        if (lane == leader) first = atomicAdd(&st->cnt[c], (u32)__popcll(m));
        first = (u32)__shfl((int)first, (int)leader);
        if (cls == c) *two_sided_at(lists, rows, c, first + (u32)__popcll(m & lanemask_lt())) = r0 + t;
    }
}

// ------------------------------------------------------------------------------------------------ rows kept whole
// The entries of the tile's rows of at most k entries, numbered through: entry j of them belongs to the row whose end (an
// inclusive scan of the lengths, LDS) is the first beyond j; s_src / s_dst turn j into its place in A's and in C's buffers.
template <typename T>
__global__ __launch_bounds__(kCopyTileRows) void topk_copy_kernel(const u32* __restrict__ ro, const u32* __restrict__ col,
                                                                  const T* __restrict__ val, const u32* __restrict__ new_ro, u32 rows, u32 k,
                                                                  u32* __restrict__ c_col, T* __restrict__ c_val, TopkStatus* __restrict__ st)
{
    SPECK_POISON();
    __shared__ u32 s_end[kCopyTileRows], s_src[kCopyTileRows], s_dst[kCopyTileRows];
    __shared__ u32 s_scan[kCopyTileRows / 64 + 1];
    __shared__ unsigned long long s_nan;
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kCopyTileRows;
    const u32 nr = min(kCopyTileRows, rows - r0);
    if (t == 0) s_nan = 0;
    u32 a = 0, len = 0, to = 0;
    if (t < nr) {
        a = ro[r0 + t];
        len = ro[r0 + t + 1] - a;
        to = new_ro[r0 + t];
        if (len > k) len = 0;  // (a class kernel's row)
    }
    u32 total;
    const u32 ex = block_exclusive_scan<kCopyTileRows>(len, s_scan, &total);
    s_end[t] = ex + len;
    s_src[t] = a - ex;  // (modulo 2^32: the sum with j is the place)
    s_dst[t] = to - ex;
    __syncthreads();
    u32 nans = 0;
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
                c[u] = col[s_src[r[u]] + j];
                v[u] = val[s_src[r[u]] + j];
            }
        }
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 j = j0 + u * kCopyTileRows + t;
            if (j < total) {
                c_col[s_dst[r[u]] + j] = c[u];
                c_val[s_dst[r[u]] + j] = v[u];
                nans += bits_are_nan(value_bits(v[u])) ? 1u : 0u;
            }
        }
    }
    block_counter_to(&st->nan_kept, nans, &s_nan);
}

// ------------------------------------------------------------------------------------------------ group rows
// Entry p of the row lies in lane p % L, register p / L of its group.  Every lane reads the row's keys from LDS one after
// the other -- the lanes of a group read one address: a broadcast -- and counts for each of its entries the larger keys
// (gt) and the equal ones in front of it (eq).  Kept: gt + eq < k.  A dropped entry with gt < k has the key of a kept one
// (the first of its equals has only the gt larger ones against it): the tie rule decided in this row.
template <typename T, u32 L>
__global__ __launch_bounds__(256) void topk_group_kernel(const u32* __restrict__ ro, const u32* __restrict__ col, const T* __restrict__ val,
                                                         const u32* __restrict__ new_ro, u32 rows, const u32* __restrict__ lists, u32 k,
                                                         u32 mode, u32* __restrict__ c_col, T* __restrict__ c_val, TopkStatus* __restrict__ st)
{
    SPECK_POISON();
    using K = typename KeyOf<T>::type;
    constexpr u32 NG = 256 / L, NP = kPer * L;
    constexpr u32 LIST = L == 8 ? LIST_G8 : L == 16 ? LIST_G16 : L == 32 ? LIST_G32 : LIST_G64;
    __shared__ K s_key[NG * NP];
    __shared__ unsigned long long s_nan, s_ties;
    if (threadIdx.x == 0) s_nan = 0, s_ties = 0;
    __syncthreads();
    const u32 gl = threadIdx.x % L, gid = threadIdx.x / L;
    const u32 gshift = lane_id() & ~(L - 1u);  // the group's first lane in its wave
    const u64 gmask = L == 64 ? ~0ull : ((1ull << L) - 1ull);
    K* mine = s_key + gid * NP;
    const u32 n_list = st->cnt[LIST];
    u32 nans = 0, ties = 0;
    for (u32 e = blockIdx.x * NG + gid; e < n_list; e += gridDim.x * NG) {
        const u32 row = *two_sided_at(lists, rows, LIST, e);
        const u32 a0 = ro[row], n = min(ro[row + 1] - a0, NP), o0 = new_ro[row];
        K key[kPer];
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 p = u * L + gl;
            key[u] = 0;
            if (p < n) {
                key[u] = key_of_bits<K>(value_bits(val[a0 + p]), mode);
                mine[p] = key[u];
            }
        }
        wave_lds_fence();
        u32 gt[kPer] = {0, 0, 0, 0}, eq[kPer] = {0, 0, 0, 0};
        for (u32 q = 0; q < n; ++q) {
            const K other = mine[q];
#pragma unroll
            for (u32 u = 0; u < kPer; ++u) {
                gt[u] += other > key[u] ? 1u : 0u;
                eq[u] += (other == key[u] && q < u * L + gl) ? 1u : 0u;
            }
        }
        u32 placed = 0;
        bool tie = false;
#pragma unroll
        for (u32 u = 0; u < kPer; ++u) {
            const u32 p = u * L + gl;
            const bool kept = p < n && gt[u] + eq[u] < k;
            tie |= p < n && !kept && gt[u] < k;
            const u64 m = (__ballot(kept) >> gshift) & gmask;
            if (kept) {
                const u32 to = o0 + placed + (u32)__popcll(m & ((1ull << gl) - 1ull));
                c_col[to] = col[a0 + p];
                c_val[to] = val[a0 + p];
                nans += key[u] == ~K(0) ? 1u : 0u;
            }
            placed += (u32)__popcll(m);
        }
        const bool row_tie = ((__ballot(tie) >> gshift) & gmask) != 0;
        if (gl == 0 && row_tie) ++ties;
        wave_lds_fence();  // the next row overwrites the keys
    }
    wave_counter_to_lds(&s_nan, nans);
    wave_counter_to_lds(&s_ties, ties);
    __syncthreads();
    lds_counter_to_status(&st->nan_kept, &s_nan, 0u);
    if (threadIdx.x == 64 && s_ties) atomicAdd(&st->ties_cut, (u32)s_ties);
}

// ------------------------------------------------------------------------------------------------ LDS rows, long rows
// an entry of the pass's candidates counts in the bin of its digit: ONE LDS atomic where the wave's candidates share the
// digit (the upper bytes of a row's keys mostly agree), one per lane elsewhere.  Whole waves.
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
__global__ __launch_bounds__(kThreads) void topk_row_kernel(const u32* __restrict__ ro, const u32* __restrict__ col, const T* __restrict__ val,
                                                            const u32* __restrict__ new_ro, u32 rows, const u32* __restrict__ lists, u32 k,
                                                            u32 mode, u32* __restrict__ c_col, T* __restrict__ c_val,
                                                            TopkStatus* __restrict__ st)
{
    SPECK_POISON();
    using K = typename KeyOf<T>::type;
    constexpr u32 kBits = sizeof(K) * 8;
    constexpr u32 LIST = kLds ? LIST_LDS : LIST_LONG;
    static_assert(kThreads >= 256 && kThreads <= 1024, "a thread per bin; a scan's counts fit 16 bits");
    __shared__ K s_key[kLds ? kLdsMax : 1];
    __shared__ u32 s_hist[256];
    __shared__ u32 s_scan[kThreads / 64 + 1];
    __shared__ u32 s_sel[3];
    __shared__ unsigned long long s_nan;
    const u32 t = threadIdx.x;
    if (t == 0) s_nan = 0;
    const u32 n_list = st->cnt[LIST];
    u32 nans = 0, ties = 0;
    for (u32 e = blockIdx.x; e < n_list; e += gridDim.x) {
        const u32 row = *two_sided_at(lists, rows, LIST, e);
        const u32 a0 = ro[row], o0 = new_ro[row];
        const u32 n = kLds ? min(ro[row + 1] - a0, kLdsMax) : ro[row + 1] - a0;
        if (kLds)
            for (u32 i = t; i < n; i += kThreads) s_key[i] = key_of_bits<K>(value_bits(val[a0 + i]), mode);
        // ---- the k-th key: `prefix` = its bytes above `shift`, `need` = the entries still to take among the keys that
        // share them (every key with larger upper bytes is taken)
        K prefix = 0;
        u32 need = k, shift = kBits, bin_cnt = 0;
        do {
            const bool first = shift == kBits;
            const u32 upper = first ? 0u : shift;  // the candidates: key >> upper == prefix
            shift -= 8;
            if (t < 256) s_hist[t] = 0;
            __syncthreads();  // (and the keys are in LDS)
            for (u64 i0 = 0; i0 < n; i0 += u64(kThreads) * kPer) {
                K key[kPer];
                bool ok[kPer];
#pragma unroll
                for (u32 u = 0; u < kPer; ++u) {
                    const u64 i = i0 + u * kThreads + t;
                    ok[u] = i < n;
                    key[u] = 0;
                    if (ok[u]) key[u] = kLds ? s_key[i] : key_of_bits<K>(value_bits(val[a0 + i]), mode);
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
            prefix = (prefix << 8) | K(s_sel[0]);
            need -= s_sel[1];
            bin_cnt = s_sel[2];
        } while (shift != 0 && bin_cnt != need);  // (the whole bin is needed: nothing is left to narrow)
        // keep key > tau, and the first tq of key == tau
        K tau = prefix;
        u32 tq = need;
        if (shift != 0) tau = (prefix << shift) - 1u, tq = 0;  // every key from prefix << shift on (> 0: fewer than n are kept)
        else if (t == 0 && bin_cnt > need) ++ties;
        // ---- the ordered walk: one packed scan (low half: key > tau, high half: key == tau) per kThreads entries
        u32 carry_gt = 0, carry_eq = 0;
        for (u64 i0 = 0; i0 < n; i0 += u64(kThreads) * kPer) {
            K key[kPer];
            bool ok[kPer];
#pragma unroll
            for (u32 u = 0; u < kPer; ++u) {
                const u64 i = i0 + u * kThreads + t;
                ok[u] = i < n;
                key[u] = 0;
                if (ok[u]) key[u] = kLds ? s_key[i] : key_of_bits<K>(value_bits(val[a0 + i]), mode);
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
                    c_col[to] = col[a0 + i];
                    c_val[to] = val[a0 + i];
                    nans += key[u] == ~K(0) ? 1u : 0u;
                }
                carry_gt += total & 0xFFFFu;
                carry_eq += total >> 16;
            }
        }
        __syncthreads();  // the next row overwrites the keys
    }
    block_counter_to(&st->nan_kept, nans, &s_nan);
    if (t == 0 && ties) atomicAdd(&st->ties_cut, ties);
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int topk_run(TopKScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_topk_params* p, speck_dcsr* C, speck_topk_info* info,
             COut* out)
{
    const u32 rows = (u32)A->rows, cols = (u32)A->cols;
    const u64 nnz = A->nnz;
    if (rows == 0) return publish_empty_c(C, A->cols, sizeof(T), s, out);
    const u32 k = (u32)std::min<u64>(p->k, 0xFFFFFFFFull);  // (a row holds fewer than 2^32 entries: such a k cuts none)
    const u32* ro = A->row_offsets;
    const u32* col = A->col_ids;
    const T* val = static_cast<const T*>(A->data);

    // status | lists (three regions of `rows` words) | kept per row | new row offsets | workgroup sums of the scan
    RowScratch<TopkStatus> f;
    int rc = carve_row_scratch(&sc->fixed, rows, size_t(3) * rows, &f);
    if (rc != SPECK_OK) return rc;
    TopkStatus* st = f.st;

    // ---- the verdict on A, the lists and nnz(C): read before anything of C is allocated or written
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(TopkStatus), s));
    if (nnz / rows >= kTopkTileLongAvg || rows < kTopkTileLongRows)
        SPECK_LAUNCH(topk_classify_kernel<kTopkTileRows>, dim3((rows + kTopkTileRows - 1) / kTopkTileRows), dim3(kClassifyThreads), 0, s, ro,
                     col, rows, cols, nnz, k, sc->group_max, sc->lds_max, f.row_cnt, f.lists, st);
    else
        SPECK_LAUNCH(topk_classify_kernel<kTopkTileRowsLong>, dim3((rows + kTopkTileRowsLong - 1) / kTopkTileRowsLong),
                     dim3(kClassifyThreads), 0, s, ro, col, rows, cols, nnz, k, sc->group_max, sc->lds_max, f.row_cnt, f.lists, st);
    // (on a refused input the counts of a tile may be missing: the scan adds up whatever the words hold and addresses
    //  nothing through them)
    launch_exclusive_scan(s, CountArray{f.row_cnt}, rows, f.block_sums, f.new_ro, &st->nnz_out);
    TopkStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid || h.entries != nnz) return SPECK_ERR_INVALID;  // (the last offset spans nnz, as for speck_select_*)

    // ---- C
    const u64 nnz_out = h.nnz_out;
    u64 rows_cut = 0;
    for (int c = 0; c < TOPK_LISTS; ++c) rows_cut += h.cnt[c];
    rc = prepare_c(C, rows, nnz_out, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    if (nnz_out) {
        u32* c_col = out->col;
        T* c_val = static_cast<T*>(out->val);
        if (rows_cut < rows)
            SPECK_LAUNCH(topk_copy_kernel<T>, dim3((rows + kCopyTileRows - 1) / kCopyTileRows), dim3(kCopyTileRows), 0, s, ro, col, val,
                         f.new_ro, rows, k, c_col, c_val, st);
        if (h.cnt[LIST_G8])
            SPECK_LAUNCH((topk_group_kernel<T, 8>), dim3(grid_of((h.cnt[LIST_G8] + 31) / 32, kGroupGrid)), dim3(256), 0, s, ro, col, val,
                         f.new_ro, rows, f.lists, k, p->mode, c_col, c_val, st);
        if (h.cnt[LIST_G16])
            SPECK_LAUNCH((topk_group_kernel<T, 16>), dim3(grid_of((h.cnt[LIST_G16] + 15) / 16, kGroupGrid)), dim3(256), 0, s, ro, col, val,
                         f.new_ro, rows, f.lists, k, p->mode, c_col, c_val, st);
        if (h.cnt[LIST_G32])
            SPECK_LAUNCH((topk_group_kernel<T, 32>), dim3(grid_of((h.cnt[LIST_G32] + 7) / 8, kGroupGrid)), dim3(256), 0, s, ro, col, val,
                         f.new_ro, rows, f.lists, k, p->mode, c_col, c_val, st);
        if (h.cnt[LIST_G64])
            SPECK_LAUNCH((topk_group_kernel<T, 64>), dim3(grid_of((h.cnt[LIST_G64] + 3) / 4, kGroupGrid)), dim3(256), 0, s, ro, col, val,
                         f.new_ro, rows, f.lists, k, p->mode, c_col, c_val, st);
        if (h.cnt[LIST_LDS])
            SPECK_LAUNCH((topk_row_kernel<T, 256, true>), dim3(grid_of(h.cnt[LIST_LDS], kLdsGrid)), dim3(256), 0, s, ro, col, val, f.new_ro,
                         rows, f.lists, k, p->mode, c_col, c_val, st);
        if (h.cnt[LIST_LONG])
            SPECK_LAUNCH((topk_row_kernel<T, 1024, false>), dim3(grid_of(h.cnt[LIST_LONG], kLongGrid)), dim3(1024), 0, s, ro, col, val,
                         f.new_ro, rows, f.lists, k, p->mode, c_col, c_val, st);
        if (info) {  // the counters of the kernels that wrote C
            rc = read_status(s, st, &h);
            if (rc != SPECK_OK) return rc;
        }
    }
    rc = finish_rows(s, f.new_ro, rows, A->cols, nnz_out, C, out);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->rows = rows;
        info->rows_cut = rows_cut;
        info->entries_in = nnz;
        info->nnz_out = nnz_out;
        info->dropped = nnz - nnz_out;
        info->max_row_entries = h.max_row;
        info->ties_cut = h.ties_cut;
        info->nan_kept = h.nan_kept;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"top-k lists and row counts", "top-k temporaries", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int topk_impl(speck_config* cfg, const speck_dcsr* A, const speck_topk_params* p, speck_dcsr* C, speck_topk_info* info)
{
    if (!A || !p || !C) return SPECK_ERR_INVALID;
    if (p->mode != SPECK_TOPK_LARGEST && p->mode != SPECK_TOPK_SMALLEST && p->mode != SPECK_TOPK_LARGEST_ABS) return SPECK_ERR_INVALID;
    if (p->reserved != 0) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    // (topk_copy_kernel numbers the kept entries of a tile of 256 rows in 32 bits and steps by 1024)
    if (A->nnz > (1ull << 32) - 1024) return SPECK_ERR_NNZ_OVERFLOW;
    if (!csr_args_ok(A, true) || (A->nnz && (A->rows == 0 || A->cols == 0))) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A)) return SPECK_ERR_INVALID;
    if (info) *info = speck_topk_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, topk_scratch, C, info, kGuardNames, " by the top-k",
                         [&](TopKScratch* sc, hipStream_t s, COut* out) { return topk_run<T>(sc, s, A, p, C, info, out); });
}

}  // namespace

extern "C" {

int speck_topk_f64(speck_config* cfg, const speck_dcsr* A, const speck_topk_params* p, speck_dcsr* C, speck_topk_info* info)
{
    return topk_impl<double>(cfg, A, p, C, info);
}

int speck_topk_f32(speck_config* cfg, const speck_dcsr* A, const speck_topk_params* p, speck_dcsr* C, speck_topk_info* info)
{
    return topk_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
