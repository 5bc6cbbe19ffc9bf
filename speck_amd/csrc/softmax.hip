// softmax.hip -- speck_softmax_*: the softmax of every row of a device CSR over the entries the row holds, p = exp(alpha a -
// m_i) / s_i (NORMALIZED) or exp(alpha a - m_i) (EXP), and its backward, alpha p (g - r_i) with r_i the row's sum of p g;
// in place or into a new C.  Every step in double, one rounding to T.  The step between speck_sddmm_* (the scores) and
// speck_spmm_* (the aggregation) of an attention layer on a graph.  The reference has no counterpart.
//
//   tile_check_kernel     (tile_combine.hpp) a thread per row: the offsets, the rows of every entry tile's first and last
//                         entry, the rows without an entry.  Raises the verdict in the status block.
//   softmax_ids_kernel    a new C only: a stream over col_ids, each < cols (compared, never followed); the same verdict.
//                         Every kernel below is queued behind the two, looks at the verdict first and does nothing where
//                         it is raised: the vectors and in-place data are written directly.
//   softmax_tile_kernel   a workgroup per ENTRY TILE of 4096 absolute entries, 16 per thread (tile_frame, load_entries).
//                         Forward: x = alpha a; combine_terms<MAX> over the x; a row that lies whole in the tile leaves
//                         its m at the place of its first entry in LDS, and a thread learns the value of its first entry's
//                         row from the last such place in front of it (a max-scan over the threads, as scale_tile_kernel
//                         finds l[i]), then walks its 16 row-start bits; e = exp(x - m); combine_terms<SUM> over the e; the
//                         row's s comes back the same way; the division; ONE store.  The entries of the rows the tile does
//                         not hold whole carry the identity in both combines and are not written; their partial maximum
//                         goes to the tile's record.  Backward: the same frame with one combine, over w = p g, whose
//                         records are complete at once.
//   softmax_finish_kernel chain_finish over the records of one monoid: a wave per tile gives the row that leaves the tile
//                         open its m (or s, or r); a thread per row gives the rows without entries the identity where the
//                         caller asked for the vector, and a new C its row offsets.
//   softmax_split_sum_kernel    forward only, the second visit: a tile with a head or a tail loads those entries alone,
//                         forms e with the row's m and combines them in the tile's tree (the whole rows' terms are the
//                         identity now); its records are what chain_finish<SUM> reads.  Returns at once elsewhere.
//   softmax_split_write_kernel  the last visit of the same tiles: e again and the division (backward: the chain with r).
// The three launches behind the first are queued unconditionally -- nothing is read back in the middle.  No kernel waits
// on another workgroup: every dependency between tiles is a kernel boundary.  Every tree is tile_combine.hpp's and depends
// on the absolute positions of the entries alone, so a row's s_i has the bits of speck_reduce_*(SUM) over the e.  No
// floating-point atomic; `nonfinite` and `rows_split` are integer counters (one atomic per workgroup).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "compact.hpp"
#include "launch.hpp"
#include "side_call.hpp"
#include "tile_call.hpp"

// every product, difference, sum and quotient is rounded to double on its own
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SOFTMAX_TILE_ENTRIES, "the header's figure");
using Max = Op<SPECK_REDUCE_MAX>;
using Sum = Op<SPECK_REDUCE_SUM>;

struct SoftmaxStatus {
    u32 invalid;  // the offsets, a column id
    u32 base;     // row_offsets[0]
    unsigned long long rows_empty, rows_split, nonfinite;
};

template <typename T>
struct SoftmaxArgs {
    const u32* ro;
    const u32* col;  // read for a new C only
    const T* src;
    const T* grad;  // BACKWARD: indexed as src
    T* dst;         // in place: src, entry p at p; C's values otherwise, entry p at p - row_offsets[0]
    u32* dst_col;   // C's column ids (null: in place)
    double *row_max, *row_sum;  // the caller's vector, or the call's scratch: the rows that leave a tile always write theirs
    u64 nnz;
    u32 rows, mode;
    u32 out_max, out_sum;  // the caller's: every row writes
    u32 aligned;           // every array above that is read or written starts on a 16-byte boundary
    double alpha;
    TileRec *rec_max, *rec_sum;
    const u32* tile_rows;
    SoftmaxStatus* st;
};

constexpr u32 kIdBlocks = 1024, kIdUnroll = 4;

__global__ __launch_bounds__(kThreads) void softmax_ids_kernel(const u32* __restrict__ ro, const u32* __restrict__ col, u32 cols, u64 nnz,
                                                               SoftmaxStatus* st)
{
    SPECK_POISON();
    if (st->invalid) return;  // (queued behind tile_check_kernel: the offsets span [base, base + nnz))
    const u64 base = ro[0];
    const u64 stride = u64(gridDim.x) * kThreads * kIdUnroll;
    bool bad = false;
    for (u64 b = u64(blockIdx.x) * kThreads * kIdUnroll; b < nnz; b += stride) {
        u32 c[kIdUnroll];
#pragma unroll
        for (u32 k = 0; k < kIdUnroll; ++k) {
            const u64 i = b + k * kThreads + threadIdx.x;
            c[k] = i < nnz ? col[base + i] : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < kIdUnroll; ++k) bad |= c[k] >= cols && b + k * kThreads + threadIdx.x < nnz;
    }
    if (bad) st->invalid = 1;
}

// ------------------------------------------------------------------------------------------------ tiles
// The entries of the tile [lo, hi) whose rows it does not hold whole: [lo, head_end) belong to the row of the tile's
// first entry, which started in front of it; [tail_start, hi) to the row of its last entry, which goes on behind it.  A
// tile inside one row: both, every entry.
struct Split {
    u64 head_end, tail_start;
    __device__ __forceinline__ bool any(u64 lo, u64 hi) const { return head_end > lo || tail_start < hi; }
    __device__ __forceinline__ bool all() const { return head_end >= tail_start; }
    __device__ __forceinline__ bool holds(u64 q) const { return q < head_end || q >= tail_start; }
};

__device__ __forceinline__ Split split_of(const u32* __restrict__ ro, u32 r_lo, u32 r_hi, u64 lo, u64 hi)
{
    const u64 s_first = ro[r_lo], e_first = ro[r_lo + 1u], s_last = ro[r_hi], e_last = ro[r_hi + 1u];
    return Split{s_first < lo ? std::min(e_first, hi) : lo, e_last > hi ? std::max(s_last, lo) : hi};
}

// what a thread of a tile knows of the row starts among its entries: its 16 bits of the bitmap tile_begin left, and one
// past the last marked place among the entries of the threads in front of it (0: none).  Behind a barrier of its own.
struct RowWalk {
    u32 bits, before;
};

__device__ __forceinline__ RowWalk row_walk(const TileLds& s, u32* s_last)
{
    const u32 t = threadIdx.x;
    const u32 bits = (s.bits[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu;
    const u32 mine = bits ? t * kPer + (31u - (u32)__clz((int)bits)) + 1u : 0u;
    s_last[t] = wave_inclusive_max(mine);
    __syncthreads();
    u32 before = (t & 63u) ? s_last[t - 1u] : 0u;
    for (u32 w = 0; w < (t >> 6); ++w) before = max(before, s_last[w * 64u + 63u]);
    return RowWalk{bits, before};
}

// the thread's 16 results: with 16-byte stores where the thread holds 16 entries of whole rows of a whole tile; one by
// one elsewhere, and only the entries `live` says
template <typename T, typename Live>
__device__ __forceinline__ void store_entries(T* __restrict__ dst, u64 q0, u64 d0, bool wide, const T* y, Live&& live)
{
    if (wide) {
        constexpr u32 N = 16 / sizeof(T);
        Vec<T, N>* out = reinterpret_cast<Vec<T, N>*>(dst + (q0 - d0));
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) {
            Vec<T, N> x;
#pragma unroll
            for (u32 j = 0; j < N; ++j) x.v[j] = y[k * N + j];
            out[k] = x;
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k)
            if (live(q0 + k)) dst[q0 + k - d0] = y[k];
    }
}

template <typename T>
__device__ __forceinline__ T rounded(double x, u32& nonfinite)
{
    const T y = (T)x;
    nonfinite += !__builtin_isfinite(y);
    return y;
}

// kBwd: A holds P, one combine over p g.  kCols: a new C, whose column ids are copied here.
template <typename T, bool kBwd, bool kCols>
__global__ __launch_bounds__(kThreads) void softmax_tile_kernel(const SoftmaxArgs<T> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    __shared__ u32 s_last[kThreads];
    __shared__ unsigned long long s_count;
    if (g.st->invalid) return;  // (the verdict of the checking pass: nothing below runs on offsets or ids it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;
    const u32 t = threadIdx.x;
    const u64 d0 = g.dst_col ? g.st->base : 0;
    const u64 q0 = f.tile0 + u64(t) * kPer;
    const bool wide = f.whole && g.aligned && d0 % 4 == 0;
    if (t == 0) s_count = 0;

    // the thread's 16 entries: their terms, the identity where the matrix does not reach
    T a[kPer];
    u32 c[kCols ? kPer : 1];
    load_entries<kCols>(f, wide, g.src, g.col, a, c);
    double v[kPer];  // forward: x, then e; backward: w
    [[maybe_unused]] double gr[kBwd ? kPer : 1];
    if constexpr (kBwd) {
        T b[kPer];
        load_entries<false>(f, wide, g.grad, nullptr, b, nullptr);
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) gr[k] = (double)b[k], v[k] = (double)a[k] * gr[k];
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) v[k] = g.alpha * (double)a[k];
    }
    if (!f.whole) {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k)
            if (!entry_in(f, k)) v[k] = kBwd ? Sum::ident() : Max::ident();
    }
    if constexpr (kCols) {
        if (wide) {
            Vec<u32, 4>* dc = reinterpret_cast<Vec<u32, 4>*>(g.dst_col + (q0 - d0));
#pragma unroll
            for (u32 k = 0; k < kPer / 4; ++k) {
                Vec<u32, 4> y;
#pragma unroll
                for (u32 j = 0; j < 4; ++j) y.v[j] = c[k * 4 + j];
                dc[k] = y;
            }
        } else {
#pragma unroll
            for (u32 k = 0; k < kPer; ++k)
                if (entry_in(f, k)) g.dst_col[q0 + k - d0] = c[k];
        }
    }

    // A whole row's m, then its s (backward: its r), waits for the row's entries at the place of its FIRST entry in
    // s_tile.val: a combine reads that array at the places of the rows' LAST entries only, and a row of one entry is
    // read and written by the same thread -- so no second array of 4096 doubles, and four workgroups per CU, not two.
    const TileRows rows = tile_begin(s_tile, g.ro, g.tile_rows, f.tile0);
    const Split sp = split_of(g.ro, rows.r_lo, rows.r_hi, f.lo, f.hi);
    const u32* const ro = g.ro;
    const u64 tile0 = f.tile0;
    const auto live = [&sp](u64 q) { return q >= sp.head_end && q < sp.tail_start; };

    RowWalk w;
    if constexpr (!kBwd) {
        double* const row_max = g.out_max ? g.row_max : nullptr;
        combine_terms<Max>(s_tile, rows, v, ro, g.rec_max + blockIdx.x, tile0, f.lo, f.hi, [&](u32 r, double val) {
            s_tile.val[val_slot((u32)(ro[r] - tile0))] = val;
            if (row_max) row_max[r] = val;
        });
        __syncthreads();
        w = row_walk(s_tile, s_last);
        double m = w.before ? s_tile.val[val_slot(w.before - 1u)] : 0.0;  // (none: a head entry, which is not live)
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            if ((w.bits >> k) & 1u) m = s_tile.val[val_slot(t * kPer + k)];
            v[k] = live(q0 + k) ? exp(v[k] - m) : Sum::ident();
        }
        __syncthreads();  // (every m was read: the next combine writes s_tile.val again)
    }
    double* const row_sum = g.out_sum ? g.row_sum : nullptr;
    combine_terms<Sum>(s_tile, rows, v, ro, g.rec_sum + blockIdx.x, tile0, f.lo, f.hi, [&](u32 r, double val) {
        s_tile.val[val_slot((u32)(ro[r] - tile0))] = val;
        if (row_sum) row_sum[r] = val;
    });
    __syncthreads();
    if constexpr (kBwd) w = row_walk(s_tile, s_last);

    u32 bad = 0;
    double s = w.before ? s_tile.val[val_slot(w.before - 1u)] : 0.0;
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        if ((w.bits >> k) & 1u) s = s_tile.val[val_slot(t * kPer + k)];
        if (live(q0 + k)) {
            double x;
            if constexpr (kBwd) {
                x = gr[k] - s;
                x = (double)a[k] * x;
                x = g.alpha * x;
            } else x = g.mode == SPECK_SOFTMAX_EXP ? v[k] : v[k] / s;
            a[k] = rounded<T>(x, bad);
        }
    }
    store_entries(g.dst, q0, d0, wide && live(q0) && live(q0 + kPer - 1u), a, live);
    block_counter_to(&g.st->nonfinite, bad, &s_count);
}

// ------------------------------------------------------------------------------------------------ finish
// kFirst: the first finish of a call counts the rows that leave their tile and gives a new C its offsets
template <int OP, bool kFirst>
__global__ __launch_bounds__(kThreads) void softmax_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 chain_blocks,
                                                                  double* __restrict__ row_val, u32 out_rows, u32* __restrict__ c_ro,
                                                                  const TileRec* __restrict__ recs, SoftmaxStatus* st)
{
    SPECK_POISON();
    using O = Op<OP>;
    __shared__ unsigned long long s_count;
    if (st->invalid) return;
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u64 base = st->base;
    if (blockIdx.x < chain_blocks) {
        if (t == 0) s_count = 0;
        __syncthreads();
        u32 row;
        double val;
        const bool found = chain_finish<O>(recs, blockIdx.x * kWaves + wid, tiles_touched(base, nnz), base / kTile, &row, &val);
        if (found && lane == 0) row_val[row] = val;
        if constexpr (kFirst) block_counter_to(&st->rows_split, (u32)(found && lane == 0), &s_count);
    } else {
        const u32 r = (blockIdx.x - chain_blocks) * kThreads + t;
        if (out_rows && r < rows && ro[r] == ro[r + 1]) row_val[r] = O::ident();
        if (kFirst && c_ro && r <= rows) c_ro[r] = ro[r] - (u32)base;
    }
}

// ------------------------------------------------------------------------------------------------ the rows that leave a tile
// The entries of this tile that `sp` holds, the others T(0): 16-byte loads where they are all of a whole tile
template <typename T>
__device__ __forceinline__ void load_split(const TileFrame& f, const Split& sp, bool wide, const T* __restrict__ data, T* a)
{
    if (wide) load_entries<false>(f, true, data, nullptr, a, nullptr);
    else {
        const u64 q0 = f.tile0 + u64(threadIdx.x) * kPer;
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 q = q0 + k;
            a[k] = (q >= f.lo && q < f.hi && sp.holds(q)) ? data[q] : T(0);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void softmax_split_sum_kernel(const SoftmaxArgs<T> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;
    const u32 r_lo = g.tile_rows[2 * blockIdx.x], r_hi = g.tile_rows[2 * blockIdx.x + 1];
    const Split sp = split_of(g.ro, r_lo, r_hi, f.lo, f.hi);
    if (!sp.any(f.lo, f.hi)) return;  // (every row of the tile was finished in its first visit)
    const u64 q0 = f.tile0 + u64(threadIdx.x) * kPer;
    T a[kPer];
    load_split(f, sp, f.whole && sp.all() && g.aligned, g.src, a);
    const double m_head = g.row_max[r_lo], m_tail = g.row_max[r_hi];
    double v[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        const u64 q = q0 + k;
        const double x = g.alpha * (double)a[k];
        v[k] = (q >= f.lo && q < f.hi && sp.holds(q)) ? exp(x - (q < sp.head_end ? m_head : m_tail)) : Sum::ident();
    }
    combine_tile<Sum>(s_tile, v, g.ro, g.tile_rows, g.rec_sum + blockIdx.x, f.tile0, f.lo, f.hi, [](u32, double) {});
}

template <typename T, bool kBwd>
__global__ __launch_bounds__(kThreads) void softmax_split_write_kernel(const SoftmaxArgs<T> g)
{
    SPECK_POISON();
    __shared__ unsigned long long s_count;
    if (g.st->invalid) return;
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;
    const u32 r_lo = g.tile_rows[2 * blockIdx.x], r_hi = g.tile_rows[2 * blockIdx.x + 1];
    const Split sp = split_of(g.ro, r_lo, r_hi, f.lo, f.hi);
    if (!sp.any(f.lo, f.hi)) return;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const u64 d0 = g.dst_col ? g.st->base : 0;
    const u64 q0 = f.tile0 + u64(threadIdx.x) * kPer;
    const bool wide = f.whole && sp.all() && g.aligned && d0 % 4 == 0;
    T a[kPer];
    load_split(f, sp, wide, g.src, a);
    [[maybe_unused]] T b[kBwd ? kPer : 1];
    if constexpr (kBwd) load_split(f, sp, wide, g.grad, b);
    const double s_head = g.row_sum[r_lo], s_tail = g.row_sum[r_hi];
    [[maybe_unused]] double m_head = 0.0, m_tail = 0.0;
    if constexpr (!kBwd) m_head = g.row_max[r_lo], m_tail = g.row_max[r_hi];
    const auto mine = [&](u64 q) { return q >= f.lo && q < f.hi && sp.holds(q); };
    u32 bad = 0;
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        const u64 q = q0 + k;
        if (!mine(q)) continue;
        const bool head = q < sp.head_end;
        double x;
        if constexpr (kBwd) {
            x = (double)b[k] - (head ? s_head : s_tail);
            x = (double)a[k] * x;
            x = g.alpha * x;
        } else {
            x = g.alpha * (double)a[k];
            x = exp(x - (head ? m_head : m_tail));
            if (g.mode != SPECK_SOFTMAX_EXP) x = x / (head ? s_head : s_tail);
        }
        a[k] = rounded<T>(x, bad);
    }
    store_entries(g.dst, q0, d0, wide, a, mine);
    block_counter_to(&g.st->nonfinite, bad, &s_count);
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, bool kBwd>
void launch_tile(bool cols, u32 tiles, hipStream_t s, const SoftmaxArgs<T>& g)
{
    if (cols) SPECK_LAUNCH((softmax_tile_kernel<T, kBwd, true>), dim3(tiles), dim3(kThreads), 0, s, g);
    else SPECK_LAUNCH((softmax_tile_kernel<T, kBwd, false>), dim3(tiles), dim3(kThreads), 0, s, g);
}

template <int OP, bool kFirst>
void launch_finish(hipStream_t s, const speck_dcsr* A, u32 max_tiles, double* row_val, bool out_rows, u32* c_ro, const TileRec* recs,
                   SoftmaxStatus* st)
{
    const u32 rows = (u32)A->rows, chain_blocks = (max_tiles + kWaves - 1) / kWaves;
    SPECK_LAUNCH((softmax_finish_kernel<OP, kFirst>), dim3(chain_blocks + rows / kThreads + 1u), dim3(kThreads), 0, s, A->row_offsets, rows,
                 A->nnz, chain_blocks, row_val, out_rows ? 1u : 0u, c_ro, recs, st);
}

template <typename T>
int softmax_run(TileScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_softmax_params* p, speck_dcsr* C,
                speck_softmax_info* info, COut* out)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz = A->nnz;
    if (rows == 0) return C ? publish_empty_c(C, A->cols, sizeof(T), s, out) : SPECK_OK;
    const bool bwd = p->mode == SPECK_SOFTMAX_BACKWARD;
    // two sets of tile records (MAX, SUM) and, where the caller keeps no vector, the m and s of the rows that leave a tile
    TileWork<SoftmaxStatus> w;
    int rc = carve_and_check(sc, s, A, 2, 2 * size_t(rows), &w);
    if (rc != SPECK_OK) return rc;
    // (nnz(C) = nnz(A) is known before the first kernel: C's buffers are taken now and handed over behind the verdict)
    if (C) {
        rc = prepare_c(C, rows, nnz, sizeof(T), out);
        if (rc != SPECK_OK) return rc;
        if (nnz)
            SPECK_LAUNCH(softmax_ids_kernel, dim3(grid_of((nnz + kThreads * kIdUnroll - 1) / (kThreads * kIdUnroll), kIdBlocks)),
                         dim3(kThreads), 0, s, A->row_offsets, A->col_ids, (u32)A->cols, nnz, w.st);
    }
    T* dst = C ? static_cast<T*>(out->val) : static_cast<T*>(A->data);
    const bool aligned = on_16_bytes(A->data) && on_16_bytes(dst) && (!bwd || on_16_bytes(p->d_G)) &&
                         (!C || (on_16_bytes(A->col_ids) && on_16_bytes(out->col)));
    TileRec *rec_max = w.recs, *rec_sum = w.recs + w.max_tiles;
    const SoftmaxArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), static_cast<const T*>(p->d_G), dst,
                           C ? out->col : nullptr, p->d_row_max ? p->d_row_max : w.sums, p->d_row_sum ? p->d_row_sum : w.sums + rows,
                           nnz, rows, p->mode, p->d_row_max ? 1u : 0u, p->d_row_sum ? 1u : 0u, aligned ? 1u : 0u, p->alpha,
                           rec_max, rec_sum, w.tile_rows, w.st};
    u32* const c_ro = C ? out->ro : nullptr;
    if (bwd) {
        if (nnz) launch_tile<T, true>(C != nullptr, w.max_tiles, s, g);
        launch_finish<SPECK_REDUCE_SUM, true>(s, A, w.max_tiles, g.row_sum, g.out_sum, c_ro, rec_sum, w.st);
        if (nnz) SPECK_LAUNCH((softmax_split_write_kernel<T, true>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
    } else {
        if (nnz) launch_tile<T, false>(C != nullptr, w.max_tiles, s, g);
        launch_finish<SPECK_REDUCE_MAX, true>(s, A, w.max_tiles, g.row_max, g.out_max, c_ro, rec_max, w.st);
        if (nnz) SPECK_LAUNCH(softmax_split_sum_kernel<T>, dim3(w.max_tiles), dim3(kThreads), 0, s, g);
        launch_finish<SPECK_REDUCE_SUM, false>(s, A, w.max_tiles, g.row_sum, g.out_sum, nullptr, rec_sum, w.st);
        if (nnz) SPECK_LAUNCH((softmax_split_write_kernel<T, false>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
    }
    // the ONE read-back of the call: the verdict, the base, the counters
    SoftmaxStatus h{};
    rc = read_status(s, w.st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    if (C) publish_c(C, rows, A->cols, nnz, out);
    if (info) {
        fill_tile_info(info, h, A);
        info->nonfinite = h.nonfinite;
    }
    return SPECK_OK;
}

const char* const kGuardNamesC[6] = {"softmax status", "softmax tile records and rows", "softmax row values", "C.data", "C.col_ids",
                                     "C.row_offsets"};
const char* const kGuardNamesA[6] = {"softmax status", "softmax tile records and rows", "softmax row values", "A.data", "A.col_ids",
                                     "A.row_offsets"};

// whether [a, a + n) and [b, b + n) doubles share a byte
bool ranges_overlap(const double* a, const double* b, u64 n)
{
    const u64 x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return (x > y ? x - y : y - x) < 8 * n;
}

template <typename T>
int softmax_impl(speck_config* cfg, const speck_dcsr* A, const speck_softmax_params* p, speck_dcsr* C, speck_softmax_info* info)
{
    if (!A || !p) return SPECK_ERR_INVALID;
    if (p->mode > SPECK_SOFTMAX_BACKWARD || p->reserved != 0) return SPECK_ERR_INVALID;
    if (!(p->alpha - p->alpha == 0.0)) return SPECK_ERR_INVALID;  // NaN, +-inf
    const bool bwd = p->mode == SPECK_SOFTMAX_BACKWARD;
    if (bwd ? (p->d_row_max != nullptr || (A->nnz && !p->d_G)) : p->d_G != nullptr) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    // (col_ids is read only for a new C: in place it may be NULL)
    if ((A->rows && !A->row_offsets) || (A->nnz && !A->data) || (A->rows == 0 && A->nnz)) return SPECK_ERR_INVALID;
    if (C && A->nnz && !A->col_ids) return SPECK_ERR_INVALID;
    const void* const given[3] = {p->d_G, p->d_row_max, p->d_row_sum};
    for (int i = 0; i < 3; ++i) {
        if (!given[i]) continue;
        if (is_one_of(given[i], A) || (C && is_one_of(given[i], C))) return SPECK_ERR_INVALID;
        for (int j = 0; j < i; ++j)
            if (given[i] == given[j]) return SPECK_ERR_INVALID;
    }
    if (p->d_row_max && p->d_row_sum && ranges_overlap(p->d_row_max, p->d_row_sum, A->rows)) return SPECK_ERR_INVALID;
    if (C && shares_buffer(C, A)) return SPECK_ERR_INVALID;
    if (info) *info = speck_softmax_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;

    TileScratch own;
    TileScratch* sc = cfg ? softmax_scratch(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    COut out;
    int rc = softmax_run<T>(sc, s, A, p, C, info, &out);
    if (rc != SPECK_OK) {
        (void)hipStreamSynchronize(s);
        out.discard();
        if (info) *info = speck_softmax_info{};
    }
    const speck_dcsr* X = C ? C : A;
    const void* whole[6] = {sc->fixed.p, sc->var.p, sc->sums.p, X->data, X->col_ids, X->row_offsets};
    rc = guard_check_buffers(whole, C ? kGuardNamesC : kGuardNamesA, 6, s, " by the softmax", rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    return rc;
}

}  // namespace

extern "C" {

int speck_softmax_f64(speck_config* cfg, const speck_dcsr* A, const speck_softmax_params* p, speck_dcsr* C, speck_softmax_info* info)
{
    return softmax_impl<double>(cfg, A, p, C, info);
}

int speck_softmax_f32(speck_config* cfg, const speck_dcsr* A, const speck_softmax_params* p, speck_dcsr* C, speck_softmax_info* info)
{
    return softmax_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
