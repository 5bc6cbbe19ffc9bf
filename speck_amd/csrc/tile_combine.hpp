// tile_combine.hpp -- the segmented combine over ENTRY TILES that reduce.hip, spmv.hip and spmm.hip share: a workgroup of 256 threads
// holds the 4096 terms of a tile, 16 consecutive ones per thread, and combines them per row -- serially in the thread,
// across the lanes with DPP shifts, across the four waves through LDS; a row that ends in the tile goes to the caller's
// sink, a row open at the tile's start or end leaves its partial in the tile's record (TileRec), and chain_finish puts
// such a row together from the records in a fixed tree over the tile numbers.  Where the 16 terms of a thread come from
// (g(a) in the reduction, a x[j] in the matrix-vector product) and what happens to a finished row is the caller's; the
// tree is one: it depends on the absolute positions of the entries alone.  The check of the offsets, which also tells
// every tile the rows of its first and last entry, is entry_tiles.hpp's behind one kernel for all three.
// Around the combine, what a tile's workgroup does first and a finish kernel does last is here as well: which entries
// the tile holds (tile_frame), the load of a thread's 16 values and column ids (load_entries), the check of an id
// (clamp_id), the status block of the two products (ProductStatus) and the one write of a y (write_y).  The host side of
// the three calls is tile_call.hpp.
#pragma once
#include <algorithm>

#include "entry_tiles.hpp"
#include "row_tiles.hpp"

// every sum is rounded on its own: all code paths add the same terms
#pragma clang fp contract(off)

namespace speck {
namespace tile_combine {

#ifdef __HIPCC__
constexpr u32 kTile = 4096, kThreads = 256, kPer = kTile / kThreads, kWaves = kThreads / 64;
static_assert(kPer == 16, "a thread's boundary bits are half a word of the bitmap");

// what a tile leaves for the rows it does not hold whole, and its own total
struct TileRec {
    double head;   // the entries in front of the first row start (the row ends here), or the whole tile where it lies inside one row
    double tail;   // the entries from the last row start on, where that row goes on behind the tile
    double total;
    u32 tail_row, tail_end;  // that row and where it ends
    u32 chain;               // the row of `tail` starts in this tile: its result is combined from here
    u32 pad_;
};

// the monoid: SPECK_REDUCE_* of speck_c_api.h (the matrix-vector product adds: SPECK_REDUCE_SUM)
template <int OP>
struct Op {
    static constexpr bool kSum = OP == SPECK_REDUCE_SUM || OP == SPECK_REDUCE_ABS_SUM || OP == SPECK_REDUCE_SQ_SUM;
    __host__ __device__ static double ident()
    {
        return OP == SPECK_REDUCE_MAX ? -__builtin_huge_val() : OP == SPECK_REDUCE_MIN ? __builtin_huge_val() : 0.0;
    }
    __device__ __forceinline__ static double term(double v)
    {
#pragma clang fp contract(off)
        if (OP == SPECK_REDUCE_ABS_SUM || OP == SPECK_REDUCE_ABS_MAX) return __builtin_fabs(v);
        if (OP == SPECK_REDUCE_SQ_SUM) return v * v;
        return v;
    }
    // (a NaN on either side comes out: `fmax` would drop it)
    __device__ __forceinline__ static double comb(double a, double b)
    {
#pragma clang fp contract(off)
        if (kSum) return a + b;
        if (OP == SPECK_REDUCE_MIN) return (a < b || a != a) ? a : b;
        return (a > b || a != a) ? a : b;
    }
};

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_move_f64(double old, double v)
{
    const u64 o = (u64)__double_as_longlong(old), x = (u64)__double_as_longlong(v);
    const u32 lo = dpp_move<CTRL, ROW_MASK>((u32)o, (u32)x), hi = dpp_move<CTRL, ROW_MASK>((u32)(o >> 32), (u32)(x >> 32));
    return __longlong_as_double((long long)((u64(hi) << 32) | lo));
}

// one step of the segmented inclusive scan: x = the combination of the lanes of my segment up to me, f = "a segment
// starts in a lane up to me".  Lanes without a source receive the identity.
template <typename O, int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ void segmented_step(double& x, u32& f)
{
    const double px = dpp_move_f64<CTRL, ROW_MASK>(O::ident(), x);
    const u32 pf = dpp_move<CTRL, ROW_MASK>(0u, f);
    x = f ? x : O::comb(px, x);
    f |= pf;
}

template <typename O>
__device__ __forceinline__ void wave_segmented_scan(double& x, u32& f)
{
    segmented_step<O, kDppRowShr + 1>(x, f);
    segmented_step<O, kDppRowShr + 2>(x, f);
    segmented_step<O, kDppRowShr + 4>(x, f);
    segmented_step<O, kDppRowShr + 8>(x, f);
    segmented_step<O, kDppRowBcast15, 0xA>(x, f);
    segmented_step<O, kDppRowBcast31, 0xC>(x, f);
}

// all 64 lanes combined, a fixed butterfly (lane 0's result is what is used)
template <typename O>
__device__ __forceinline__ double wave_combine(double x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = O::comb(x, __shfl_xor(x, m));
    return x;
}

// ------------------------------------------------------------------------------------------------ check
// the status block of spmv.hip and spmm.hip (reduce.hip's carries a total instead of bad_id)
struct ProductStatus {
    u32 invalid;  // the offsets (tile_check_kernel)
    u32 base;     // row_offsets[0]
    unsigned long long rows_empty, rows_split;
    u32 bad_id;   // a column id >= cols (the tile kernel)
};

// A thread per row (entry_tiles.hpp); Status begins with { u32 invalid, base; unsigned long long rows_empty; }.
// tile_rows[2 i], [2 i + 1]: the rows of the first and of the last entry of the i-th tile the matrix touches
template <typename Status>
__global__ __launch_bounds__(kThreads) void tile_check_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 max_tiles,
                                                              u32* __restrict__ tile_rows, Status* st)
{
    SPECK_POISON();
    __shared__ unsigned long long s_empty;
    const u32 r = blockIdx.x * kThreads + threadIdx.x;
    const u32 base = ro[0];
    if (threadIdx.x == 0) s_empty = 0;
    if (r == 0) st->base = base;
    __syncthreads();
    bool empty = false;
    if (r < rows && !row_offsets_sound<kTile>(ro, r, rows, base, nnz, max_tiles, tile_rows, &empty)) st->invalid = 1;
    block_counter_to(&st->rows_empty, (u32)empty, &s_empty);
}

// ------------------------------------------------------------------------------------------------ tiles
// The tile of workgroup i: the absolute entries [tile0, tile0 + kTile), of which [lo, hi) belong to the matrix -- all of
// them where `whole`
struct TileFrame {
    u64 tile0, lo, hi;
    bool whole;
};

// The i-th tile a matrix of nnz entries from `base` on touches; false where it touches fewer: this workgroup has no tile
// (the grid is sized without knowing the base).  The forms of this function, of entry_in and of clamp_id are the ones that
// leave the tile kernels their registers: DESIGN.md 4.18.
__device__ __forceinline__ bool tile_frame(u64 base, u64 nnz, u32 i, TileFrame* f)
{
    const u64 end = base + nnz, tile0 = (base / kTile + i) * kTile;
    const u64 lo = std::max(tile0, base), hi = std::min(tile0 + kTile, end);
    *f = TileFrame{tile0, lo, hi, lo == tile0 && hi == tile0 + kTile};
    return tile0 < end;
}

template <typename V, u32 N>
struct alignas(16) Vec {
    V v[N];
};

// The thread's kPer entries of the tile, the absolute entries from f.tile0 + kPer threadIdx.x on: their values in a and,
// with IDS, their column ids in c (without: c is not touched and may be null).  wide: 16-byte loads -- the caller says
// that the tile is whole and that the arrays lie on 16-byte boundaries; entry by entry elsewhere, and where the matrix
// does not reach the value is T(0) and the id 0.
template <bool IDS, typename T>
__device__ __forceinline__ void load_entries(const TileFrame& f, bool wide, const T* __restrict__ data, const u32* __restrict__ col,
                                             T* a, u32* c)
{
    const u64 q0 = f.tile0 + u64(threadIdx.x) * kPer;
    if (wide) {
        constexpr u32 N = 16 / sizeof(T);
        const Vec<T, N>* src = reinterpret_cast<const Vec<T, N>*>(data + q0);
        Vec<T, N> av[kPer / N];
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) av[k] = src[k];
        if constexpr (IDS) {
            const Vec<u32, 4>* cs = reinterpret_cast<const Vec<u32, 4>*>(col + q0);
            Vec<u32, 4> cv[kPer / 4];
#pragma unroll
            for (u32 k = 0; k < kPer / 4; ++k) cv[k] = cs[k];
#pragma unroll
            for (u32 k = 0; k < kPer; ++k) c[k] = cv[k / 4].v[k % 4];
        }
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) a[k] = av[k / N].v[k % N];
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            const bool in = p >= f.lo && p < f.hi;
            a[k] = in ? data[p] : T(0);
            if constexpr (IDS) c[k] = in ? col[p] : 0u;
        }
    }
}

// The column ids alone, as load_entries<true> leaves them in c, for a caller that never reads the values (the SECOND
// semirings of semiring.hip: A->data may be null).  wide: the tile is whole and col lies on a 16-byte boundary.
__device__ __forceinline__ void load_ids(const TileFrame& f, bool wide, const u32* __restrict__ col, u32* c)
{
    const u64 q0 = f.tile0 + u64(threadIdx.x) * kPer;
    if (wide) {
        const Vec<u32, 4>* cs = reinterpret_cast<const Vec<u32, 4>*>(col + q0);
        Vec<u32, 4> cv[kPer / 4];
#pragma unroll
        for (u32 k = 0; k < kPer / 4; ++k) cv[k] = cs[k];
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) c[k] = cv[k / 4].v[k % 4];
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            c[k] = (p >= f.lo && p < f.hi) ? col[p] : 0u;
        }
    }
}

// whether entry k of the thread (load_entries) lies in [lo, hi) -- in a tile that is not whole, the entries the matrix
// reaches: the term of any other is the identity
__device__ __forceinline__ bool entry_in(const TileFrame& f, u32 k)
{
    const u64 p = f.tile0 + u64(threadIdx.x) * kPer + k;
    return p >= f.lo && p < f.hi;
}

// An id the matrix has no column for is reported and not followed: the id a gather may use, with `bad` raised where c
// lies behind `last`, the matrix's last column
__device__ __forceinline__ u32 clamp_id(u32 c, u32 last, bool* bad)
{
    *bad |= c > last;
    return std::min(c, last);
}

// the LDS of a tile's workgroup (about 36 KB)
struct TileLds {
    double val[kTile + kTile / 16];
    double incl[kThreads];
    double wave[kWaves], wtot[kWaves];
    u32 wflag[kWaves];
    u32 bits[kTile / 32];
};

// where the running value at entry i of the tile rests in LDS (a thread's 16 entries 17 doubles apart: two lanes per bank)
__device__ __forceinline__ u32 val_slot(u32 i) { return i + (i >> 4); }

// The rows of the tile's first and last entry: what a tile's workgroup works out ONCE, whatever number of term vectors it
// combines afterwards (tile_begin)
struct TileRows {
    u32 r_lo, r_hi;
};

// Once per tile: the rows of the tile's first and last entry (tile_check_kernel) and the row starts inside the tile
// [tile0, tile0 + kTile) as a bitmap in s.bits, which every combine_terms that follows reads.  All 256 threads call it;
// it ends behind a barrier.
__device__ __forceinline__ TileRows tile_begin(TileLds& s, const u32* __restrict__ ro, const u32* __restrict__ tile_rows, u64 tile0)
{
    const u32 t = threadIdx.x;
    if (t < kTile / 32) s.bits[t] = 0;
    const u32 r_lo = tile_rows[2 * blockIdx.x], r_hi = tile_rows[2 * blockIdx.x + 1];
    __syncthreads();
    for (u64 r = u64(r_lo) + t; r <= u64(r_hi) + 1; r += kThreads) {
        const u64 o = ro[r];
        if (o >= tile0 && o < tile0 + kTile) atomicOr(&s.bits[(u32)(o - tile0) >> 5], 1u << ((u32)(o - tile0) & 31u));
    }
    __syncthreads();
    return TileRows{r_lo, r_hi};
}

// The combine of ONE vector of terms of the tile tile_begin prepared, the absolute entries [tile0, tile0 + kTile) of which
// [lo, hi) belong to the matrix: v holds the terms of the thread's 16 entries, the identity where the matrix does not
// reach.  row_done(r, val) receives every row that lies whole in the tile (rows without entries: the caller's own pass);
// rec receives the rest.  All 256 threads call it; the offsets were checked.  It leaves s.val and s.incl in use by the
// threads that are still collecting their rows: a caller that combines another vector puts a barrier in between.
template <typename O, typename RowDone>
__device__ __forceinline__ void combine_terms(TileLds& s, const TileRows rows, const double (&v)[kPer], const u32* __restrict__ ro,
                                              TileRec* rec, u64 tile0, u64 lo, u64 hi, RowDone&& row_done)
{
#pragma clang fp contract(off)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u32 r_lo = rows.r_lo, r_hi = rows.r_hi;

    // in the thread: the running value restarts at every row start; what it was in front of one, and at the thread's
    // last entry, goes to LDS
    const u32 bits = (s.bits[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu;
    double acc = O::ident(), tot = O::ident();
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        if ((bits >> k) & 1u) {
            if (k) s.val[val_slot(t * kPer + k - 1u)] = acc;
            acc = O::ident();
        }
        acc = O::comb(acc, v[k]);
        tot = O::comb(tot, v[k]);
    }
    s.val[val_slot(t * kPer + kPer - 1u)] = acc;

    // across the threads: segmented by "a row starts in this thread"
    double x = acc;
    u32 f = bits != 0;
    wave_segmented_scan<O>(x, f);
    tot = wave_combine<O>(tot);
    if (lane == 63) s.wave[wid] = x, s.wflag[wid] = f;
    if (lane == 0) s.wtot[wid] = tot;
    __syncthreads();
    double carry = O::ident();
    for (u32 u = 0; u < wid; ++u) carry = s.wflag[u] ? s.wave[u] : O::comb(carry, s.wave[u]);
    s.incl[t] = f ? x : O::comb(carry, x);
    __syncthreads();

    // the rows that end in the tile
    for (u64 r = u64(r_lo) + t; r <= r_hi; r += kThreads) {
        const u64 b = ro[r], e = ro[r + 1];
        if (b == e || e > hi) continue;  // (e > lo: r >= r_lo)
        const u32 le = (u32)(e - 1 - tile0), te = le >> 4;
        double val = s.val[val_slot(le)];
        if (b < tile0 + u64(te) * kPer) val = O::comb(te ? s.incl[te - 1u] : O::ident(), val);
        if (b < lo) rec->head = val;
        else row_done((u32)r, val);
    }
    if (t == 0) {
        const u64 s_first = ro[r_lo], e_last = ro[r_hi + 1u];
        const bool head = s_first < lo, tail = e_last > hi, whole = head && tail && r_lo == r_hi;
        if (whole) rec->head = s.incl[kThreads - 1u];
        rec->tail = s.incl[kThreads - 1u];
        rec->tail_row = r_hi;
        rec->tail_end = (u32)e_last;
        rec->chain = tail && !whole;
        double total = s.wtot[0];
        for (u32 u = 1; u < kWaves; ++u) total = O::comb(total, s.wtot[u]);
        rec->total = total;
    }
}

// The workgroup of tile `i` = blockIdx.x with one vector of terms: the two above in sequence.
template <typename O, typename RowDone>
__device__ __forceinline__ void combine_tile(TileLds& s, const double (&v)[kPer], const u32* __restrict__ ro,
                                             const u32* __restrict__ tile_rows, TileRec* rec, u64 tile0, u64 lo, u64 hi,
                                             RowDone&& row_done)
{
    const TileRows rows = tile_begin(s, ro, tile_rows, tile0);
    combine_terms<O>(s, rows, v, ro, rec, tile0, lo, hi, row_done);
}

// ------------------------------------------------------------------------------------------------ finish
// the tiles a matrix of nnz entries from `base` on touches
__host__ __device__ __forceinline__ u32 tiles_touched(u64 base, u64 nnz)
{
    return nnz ? (u32)((base + nnz - 1) / kTile - base / kTile + 1) : 0u;
}

// A wave for tile i: the row that leaves it open = its tail, the whole tiles inside the row (a lane takes every 64th,
// then the butterfly), the head of the tile it ends in.  False where no row starts in the tile and goes on behind it.
template <typename O>
__device__ __forceinline__ bool chain_finish(const TileRec* __restrict__ recs, u32 i, u32 ntiles, u64 t_first, u32* row, double* val)
{
#pragma clang fp contract(off)
    if (i >= ntiles || !recs[i].chain) return false;
    const u32 lane = lane_id();
    const u32 ib = (u32)((u64(recs[i].tail_end) - 1) / kTile - t_first);
    double mid = O::ident();
    for (u32 j = i + 1u + lane; j < ib; j += 64u) mid = O::comb(mid, recs[j].head);
    mid = wave_combine<O>(mid);
    *val = O::comb(O::comb(recs[i].tail, mid), recs[ib].head);
    *row = recs[i].tail_row;
    return true;
}

// One workgroup: the tile totals in a fixed tree and the number of split rows; thread 0 returns true and holds both.
// (one atomic per split row on one word of global memory was the longest thing in the call)
template <typename O>
__device__ __forceinline__ bool totals_finish(const TileRec* __restrict__ recs, u32 ntiles, double* s_w, u32* s_split, double* total,
                                              u32* split_rows)
{
#pragma clang fp contract(off)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    double acc = O::ident();
    u32 split = 0;
    for (u32 j = t; j < ntiles; j += kThreads) acc = O::comb(acc, recs[j].total), split += recs[j].chain;
    acc = wave_combine<O>(acc);
    split = wave_reduce_add(split);
    if (lane == 0) s_w[wid] = acc, s_split[wid] = split;
    __syncthreads();
    if (t != 0) return false;
    double sum = s_w[0];
    for (u32 u = 1; u < kWaves; ++u) sum = O::comb(sum, s_w[u]), split += s_split[u];
    *total = sum;
    *split_rows = split;
    return true;
}

// y[at] = alpha s + beta y[at], each product and the sum rounded on its own; the one write of a result of spmv.hip, spmm.hip
// and spmm_t.hip.  Y: double, or float for the float blocks of the two products -- what y holds is widened where it is
// read, and the result is rounded to Y ONCE, at the store.
template <typename Y>
__device__ __forceinline__ void write_y(Y* __restrict__ y, u64 at, double s, double alpha, double beta)
{
#pragma clang fp contract(off)
    const double as = alpha * s;
    if (beta == 0.0) y[at] = (Y)as;  // (y is not read: what it held does not survive)
    else {
        const double by = beta * (double)y[at];
        y[at] = (Y)(as + by);
    }
}

// N elements of a dense block in one load of N sizeof(V) bytes: 16 for two doubles or four floats, 8 for two floats
template <typename V, u32 N>
struct alignas(N * sizeof(V)) BlockVec {
    V v[N];
};
#endif  // __HIPCC__

}  // namespace tile_combine
}  // namespace speck
