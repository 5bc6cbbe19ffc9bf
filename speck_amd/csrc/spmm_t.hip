// spmm_t.hip -- speck_spmm_t_*: Y = alpha A^T X + beta Y on a device CSR through a speck_tplan (extras.hip makes it: the
// pattern of A sorted by column ONCE), X (rows x k) and Y (cols x k) row-major device arrays of doubles.  The fourth
// operation on entry tiles: the plan's t_ro is the row structure of A^T from 0, so spmm.hip's walk runs
// over it unchanged -- the same tiles, the same combination tree per column -- and column c of Y is bit for bit what
// speck_spmm_* writes on speck_transpose_*(A).  What differs is where a tile's entries come from: not 16 consecutive
// values and ids but 16 GATHERS through t_pos, and the ids of A are not followed but COMPARED: the plan is verified,
// exactly, in every call.  The reference has no counterpart.
//
//   tile_check_kernel     (tile_combine.hpp) on t_ro: the empty columns, the columns of every tile's first and last entry.
//   plan_match_kernel     a thread per row of A: row_offsets[i] - row_offsets[0] against the plan's ro0[i]; a difference
//                         raises `invalid`.  It also leaves row_offsets[0], which only a matching A gets used with.
//   spmm_t_tile_kernel    queued behind both, looks at that verdict first.  A workgroup per tile of 4096 PLAN entries from
//                         0; a thread loads its 16 t_pos and 16 t_row (16-byte loads: the plan's arrays are the library's,
//                         aligned and padded to the tile), issues the 16 value gathers data[base + t_pos], the 16 id
//                         gathers col_ids[base + t_pos] and the X gathers of the FIRST column block -- they depend on
//                         t_row alone -- before anything uses any of them; t_pos is dead from there on.  Then the tile's
//                         row-start bitmap (tile_begin), the column every entry lies in according to t_ro (the way
//                         scale.hip and sddmm.hip find an entry's row) compared with the id A holds there -- a difference
//                         raises `bad_id` -- and spmm.hip's column blocks over X(t_row, c0 ..).
//   spmm_t_finish_kernel  spmm_finish_kernel's sibling over (t_ro, cols) (sharing it would have changed spmm.hip): queued
//                         last, it sees the verdict of EVERY tile, and only it writes Y.
// t_pos < nnz and t_row < rows are the library's own; nothing of the caller's is ever used as an index.
//
// speck_spmm_t_*_b32: X and Y in float (B = float below), as spmm.hip has them: the same kernels with the block type as a
// template parameter, an element of X widened where its term is formed, Y rounded to float once in write_y, blocks of
// kCB32 columns loaded 16, 8 or 4 bytes at a time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "launch.hpp"
#include "tile_call.hpp"
#include "tplan.hpp"

// every product and every sum is rounded on its own: the terms and the sums are those of spmm.hip
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SPMV_TILE_ENTRIES && kTile == kPlanTile, "the plan is padded to spmv's tiles");
using Sum = Op<SPECK_REDUCE_SUM>;

constexpr u32 kCB = SPECK_SPMM_COLUMN_BLOCK;
static_assert(kCB % 2 == 0, "a 16-byte gather takes two columns");
// the same for float blocks (SPECK_SPMM_B32_FORCE_BLOCK: measurement builds only, profiles/blocks32.txt)
#ifdef SPECK_SPMM_B32_FORCE_BLOCK
constexpr u32 kCB32 = SPECK_SPMM_B32_FORCE_BLOCK;
#else
constexpr u32 kCB32 = SPECK_SPMM_COLUMN_BLOCK_B32;
#endif
static_assert(kCB32 % 4 == 0, "a 16-byte gather takes four columns");

// tile_check_kernel's contract, then the product's own words
struct SpmmTStatus {
    u32 invalid;  // A's offsets are not the plan's (plan_match_kernel)
    u32 base;     // t_ro[0] = 0
    unsigned long long rows_empty, rows_split;  // of A^T: the empty and the split columns of A
    u32 bad_id;   // an id of A that is not the column the plan has the entry in (the tile kernel)
    u32 a_base;   // A->row_offsets[0]
};

template <typename T, typename B = double>
struct SpmmTArgs {
    const u32* t_ro;
    const u32* t_row;
    const u32* t_pos;
    const u32* col;  // A's, only compared
    const T* data;
    const B* x;
    double* sums;  // cols k doubles: s(j,c) of the columns that lie whole in one tile
    u64 nnz, ldx;
    u32 k;          // >= 1
    u32 max_tiles;  // the records of column c start at recs + c max_tiles
    u32 pairs;      // x starts on a 16-byte boundary and ldx is even (B = float: the elements of the widest aligned load, 4, 2 or 1)
    TileRec* recs;
    const u32* tile_rows;
    SpmmTStatus* st;
};

// ------------------------------------------------------------------------------------------------ the plan against A
__global__ __launch_bounds__(kThreads) void plan_match_kernel(const u32* __restrict__ a_ro, const u32* __restrict__ ro0, u32 rows,
                                                              SpmmTStatus* st)
{
    SPECK_POISON();
    const u32 r = blockIdx.x * kThreads + threadIdx.x;  // rows + 1 <= 2^27 + 1 offsets
    const u32 base = a_ro[0];
    if (r == 0) st->a_base = base;
    // (64-bit: an offset that wrapped is a difference, and base + nnz stays below 2^32 where every offset matches)
    if (r <= rows && u64(a_ro[r]) != u64(base) + ro0[r]) st->invalid = 1;
}

// ------------------------------------------------------------------------------------------------ tiles
// spmm.hip's column block with the gather rows taken from t_row: the columns [c0, c0 + W) of the tile; all 16 W gathers
// X[row ldx + c0 ..) are issued, then `between` runs -- for a tile's first block: everything that uses the gathered values
// and ids for the first time, so they and the X gathers are in flight together; nothing afterwards -- then per column the
// terms and the segmented combine, with a barrier before the next column takes the LDS.  rows, a and in_mask are
// references to the kernel's own variables: the first block's `between` is what fills them.
template <u32 W, u32 VW, typename T, typename B, typename Between>
__device__ __forceinline__ void column_block(const SpmmTArgs<T, B>& g, TileLds& s_tile, const TileRows& rows, const double (&a)[kPer],
                                             u32 (&row)[kPer], const u32& in_mask, const TileFrame& f, u32 c0, Between&& between)
{
#pragma clang fp contract(off)
    static_assert(W % VW == 0 && VW * sizeof(B) <= 16, "whole loads of at most 16 bytes");
    // (the rows pass through an empty asm: the 16 addresses derived from them are computed per block, not kept)
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) asm volatile("" : "+v"(row[e]));
    B xv[W][kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) {
        const B* src = g.x + (u64(row[e]) * g.ldx + c0);
        if (VW > 1) {
#pragma unroll
            for (u32 j = 0; j < W; j += VW) {
                const BlockVec<B, VW> p = reinterpret_cast<const BlockVec<B, VW>*>(src)[j / VW];
#pragma unroll
                for (u32 i = 0; i < VW; ++i) xv[j + i][e] = p.v[i];
            }
        } else {
#pragma unroll
            for (u32 j = 0; j < W; ++j) xv[j][e] = src[j];
        }
    }
    between();
    double* const sums = g.sums;
    const u32 nk = g.k;
#pragma unroll
    for (u32 j = 0; j < W; ++j) {
        double v[kPer];
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) v[e] = ((in_mask >> e) & 1u) ? a[e] * (double)xv[j][e] : Sum::ident();
        const u32 cc = c0 + j;
        combine_terms<Sum>(s_tile, rows, v, g.t_ro, g.recs + (u64(cc) * g.max_tiles + blockIdx.x), f.tile0, f.lo, f.hi,
                           [sums, nk, cc](u32 r, double val) { sums[u64(r) * nk + cc] = val; });
        __syncthreads();
    }
}

template <typename T, typename B>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void spmm_t_tile_kernel(const SpmmTArgs<T, B> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    __shared__ u32 s_col[kTile];      // at the place of a column's first entry: the column
    __shared__ u32 s_last[kThreads];  // one past the last such place among the entries of the threads up to t (0: none)
    if (g.st->invalid) return;  // (the verdicts on t_ro and on A's offsets: nothing below runs on an A the plan does not fit)
    TileFrame f;
    if (!tile_frame(0, g.nnz, blockIdx.x, &f)) return;
    const u32 t = threadIdx.x;
    const u64 base = g.st->a_base;

    // the thread's 16 plan entries: where each lies in A and the row it has there (zeros behind nnz: A's first entry,
    // row 0 -- loaded, never used)
    u32 pos[kPer], row[kPer];
    {
        const u64 q0 = f.tile0 + u64(t) * kPer;
        const Vec<u32, 4>* ps = reinterpret_cast<const Vec<u32, 4>*>(g.t_pos + q0);
        const Vec<u32, 4>* rs = reinterpret_cast<const Vec<u32, 4>*>(g.t_row + q0);
        Vec<u32, 4> pv[kPer / 4], rv[kPer / 4];
#pragma unroll
        for (u32 j = 0; j < kPer / 4; ++j) pv[j] = ps[j], rv[j] = rs[j];
#pragma unroll
        for (u32 j = 0; j < kPer; ++j) pos[j] = pv[j / 4].v[j % 4], row[j] = rv[j / 4].v[j % 4];
    }
    // the gathers of the values and of the ids, all issued before the first is used; t_pos is dead behind them
    T at[kPer];
    u32 id[kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) {
        const u64 p = base + pos[e];
        at[e] = g.data[p];
        id[e] = g.col[p];
    }

    double a[kPer];
    u32 in_mask = 0xFFFFu;
    TileRows rows{};
    // what the first column block runs behind its X gathers: the bitmap, the column of every entry, the comparison
    const auto first_use = [&]() {
        if (!f.whole) {
            in_mask = 0;
#pragma unroll
            for (u32 e = 0; e < kPer; ++e) in_mask |= u32(entry_in(f, e)) << e;
        }
        rows = tile_begin(s_tile, g.t_ro, g.tile_rows, f.tile0);
        // every column between the tile's first and last that holds an entry and starts in the tile names itself at the
        // place of its first entry (several empty columns may share a start with it: their bit is its bit)
        for (u64 r = u64(rows.r_lo) + t; r <= rows.r_hi; r += kThreads) {
            const u64 o = g.t_ro[r], e = g.t_ro[r + 1];
            if (o < e && o >= f.tile0 && o < f.tile0 + kTile) s_col[(u32)(o - f.tile0)] = (u32)r;
        }
        const u32 bits = (s_tile.bits[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu;
        const u32 mine = bits ? t * kPer + (31u - (u32)__clz((int)bits)) + 1u : 0u;
        s_last[t] = wave_inclusive_max(mine);
        __syncthreads();
        // the column of the thread's first entry: the last marked place in front of it, across the threads
        u32 before = (t & 63u) ? s_last[t - 1u] : 0u;
        for (u32 w = 0; w < (t >> 6); ++w) before = max(before, s_last[w * 64u + 63u]);
        u32 cur = before ? s_col[before - 1u] : rows.r_lo;  // (none: the column that holds the tile's first entry)
        bool bad = false;
#pragma unroll
        for (u32 j = 0; j < kPer; ++j) {
            // (a bit behind the matrix's last entry marks its end: no column starts there, and no entry is compared)
            if (((bits & in_mask) >> j) & 1u) cur = s_col[t * kPer + j];
            bad |= ((in_mask >> j) & 1u) && id[j] != cur;
        }
        if (bad) g.st->bad_id = 1;
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) a[e] = (double)at[e];
    };
    const auto nothing = []() {};

    // the columns in blocks of kCB, then what is left in pairs and alone, as spmm.hip; the first block of whichever form
    // carries first_use
    const u32 nk = g.k;
    u32 c0;
    if constexpr (sizeof(B) == 8) {
        if (g.pairs && nk >= kCB) column_block<kCB, 2>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = kCB;
        else if (g.pairs && nk >= 2) column_block<2, 2>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = 2;
        else if (!g.pairs && nk >= kCB) column_block<kCB, 1>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = kCB;
        else column_block<1, 1>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = 1;
        if (g.pairs) {
            for (; c0 + kCB <= nk; c0 += kCB) column_block<kCB, 2>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
            for (; c0 + 2 <= nk; c0 += 2) column_block<2, 2>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
        } else {
            for (; c0 + kCB <= nk; c0 += kCB) column_block<kCB, 1>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
        }
    } else {
        // (c0 stays a multiple of the load's width: blocks of kCB32, then four, then two columns)
        const u32 vw = g.pairs;
        if (nk >= kCB32) {
            if (vw == 4) column_block<kCB32, 4>(g, s_tile, rows, a, row, in_mask, f, 0, first_use);
            else if (vw == 2) column_block<kCB32, 2>(g, s_tile, rows, a, row, in_mask, f, 0, first_use);
            else column_block<kCB32, 1>(g, s_tile, rows, a, row, in_mask, f, 0, first_use);
            c0 = kCB32;
        } else if (vw >= 2 && nk >= 2) column_block<2, 2>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = 2;
        else column_block<1, 1>(g, s_tile, rows, a, row, in_mask, f, 0, first_use), c0 = 1;
        if (vw == 4) {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 4>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
            if constexpr (kCB32 > 4)
                for (; c0 % 4 == 0 && c0 + 4 <= nk; c0 += 4) column_block<4, 4>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
        } else if (vw == 2) {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 2>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
        } else {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 1>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
        }
        if (vw >= 2)
            for (; c0 + 2 <= nk; c0 += 2) column_block<2, 2>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
    }
    for (; c0 < nk; ++c0) column_block<1, 1>(g, s_tile, rows, a, row, in_mask, f, c0, nothing);
}

// ------------------------------------------------------------------------------------------------ finish, and Y
// spmm_finish_kernel over (t_ro, cols): a wave per (tile, column of Y) finishes the column of A that leaves the tile open;
// a thread per (column of A, column of Y) writes one that lies in one tile (from `sums`) or holds no entry (+0.0); one
// workgroup counts the split columns.  Every Y(j,c) is written once by one thread, which reads it itself where beta != 0.
template <typename B>
__global__ __launch_bounds__(kThreads) void spmm_t_finish_kernel(const u32* __restrict__ t_ro, u32 cols, u64 nnz, u32 k, u32 max_tiles,
                                                                 u32 chain_blocks, u32 row_blocks, const double* __restrict__ sums,
                                                                 const TileRec* __restrict__ recs, double alpha, double beta,
                                                                 B* __restrict__ y, u64 ldy, SpmmTStatus* st)
{
    SPECK_POISON();
    __shared__ double s_w[kWaves];
    __shared__ u32 s_split[kWaves];
    if (st->invalid || st->bad_id) return;  // (every tile has run: the verdict is complete, and nothing of Y was written)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u32 ntiles = tiles_touched(0, nnz);
    if (blockIdx.x < chain_blocks) {
        const u64 w = u64(blockIdx.x) * kWaves + wid;
        const u32 c = (u32)(w / max_tiles), i = (u32)(w - u64(c) * max_tiles);
        u32 row;
        double val;
        if (c < k && chain_finish<Sum>(recs + u64(c) * max_tiles, i, ntiles, 0, &row, &val) && lane == 0)
            write_y(y, u64(row) * ldy + c, val, alpha, beta);
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        const u64 first = u64(blockIdx.x - chain_blocks) * kThreads;
        const u64 r0 = first / k;
        const u32 in = (u32)(first - r0 * k) + t;  // < k + 256
        const u64 r64 = r0 + in / k;
        const u32 c = in % k;
        if (r64 >= cols) return;
        const u32 r = (u32)r64;
        const u32 b = t_ro[r], e = t_ro[r + 1];
        if (b == e) write_y(y, u64(r) * ldy + c, Sum::ident(), alpha, beta);
        else if (b / kTile == (e - 1u) / kTile) write_y(y, u64(r) * ldy + c, sums[u64(r) * k + c], alpha, beta);  // (else: the chain above)
    } else {
        double total;
        u32 split;
        if (totals_finish<Sum>(recs, ntiles, s_w, s_split, &total, &split)) st->rows_split = split;
    }
}

// ------------------------------------------------------------------------------------------------ host
// the widest load every X(i, c) with c a multiple of its width is aligned to, as SpmmTArgs::pairs has it
inline u32 gather_width(const double* d_X, u64 ldx) { return on_16_bytes(d_X) && ldx % 2 == 0 ? 1u : 0u; }
inline u32 gather_width(const float* d_X, u64 ldx)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_X);
    return at % 16 == 0 && ldx % 4 == 0 ? 4u : at % 8 == 0 && ldx % 2 == 0 ? 2u : 1u;
}

template <typename T, typename B>
int spmm_t_run(TileScratch* sc, hipStream_t s, const speck_tplan* plan, double alpha, const speck_dcsr* A, const B* d_X, u64 ldx,
               u32 k, double beta, B* d_Y, u64 ldy, SpmmTStatus* h)
{
    const u32 rows = (u32)plan->rows, cols = (u32)plan->cols;
    // the plan's transposed structure as a matrix: what carve_and_check sizes the scratch for and checks
    speck_dcsr At{};
    At.rows = plan->cols, At.cols = plan->rows, At.nnz = plan->nnz;
    At.row_offsets = const_cast<u32*>(plan->t_ro);
    TileWork<SpmmTStatus> w;
    int rc = carve_and_check(sc, s, &At, k, size_t(cols) * k, &w);
    if (rc != SPECK_OK) return rc;
    if (rows) SPECK_LAUNCH(plan_match_kernel, dim3(rows / kThreads + 1u), dim3(kThreads), 0, s, A->row_offsets, plan->ro0, rows, w.st);
    const u32 ntiles = tiles_touched(0, plan->nnz);  // (the plan starts at 0: the tiles are known here)
    if (ntiles) {
        const SpmmTArgs<T, B> g{plan->t_ro, plan->t_row, plan->t_pos, A->col_ids, static_cast<const T*>(A->data), d_X, w.sums, plan->nnz,
                                ldx, k, w.max_tiles, gather_width(d_X, ldx), w.recs, w.tile_rows, w.st};
        SPECK_LAUNCH((spmm_t_tile_kernel<T, B>), dim3(ntiles), dim3(kThreads), 0, s, g);
    }
    // (cols <= 2^27, k <= 2^10, tiles <= 2^20 + 1: the grid stays below 2^30)
    const u32 chain_blocks = (u32)((u64(w.max_tiles) * k + kWaves - 1) / kWaves);
    const u32 row_blocks = (u32)((u64(cols) * k + kThreads - 1) / kThreads);
    SPECK_LAUNCH(spmm_t_finish_kernel<B>, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, plan->t_ro, cols, plan->nnz, k,
                 w.max_tiles, chain_blocks, row_blocks, w.sums, w.recs, alpha, beta, d_Y, ldy, w.st);
    // the ONE read-back of the call: the two verdicts, the counters
    rc = read_status(s, w.st, h);
    if (rc != SPECK_OK) return rc;
    return (h->invalid || h->bad_id) ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kGuardNames[3] = {"spmm_t status", "spmm_t tile records and columns", "spmm_t column sums"};

template <typename T, typename B>
int spmm_t_impl(speck_config* cfg, const speck_tplan* plan, double alpha, const speck_dcsr* A, const B* d_X, u64 ldx, u32 k,
                double beta, B* d_Y, u64 ldy, speck_spmm_t_info* info)
{
    if (!plan || !A || alpha != alpha || beta != beta) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || k > SPECK_SPMM_MAX_RHS) return SPECK_ERR_DIM_LIMIT;
    if (ldx > (1ull << 32) || ldy > (1ull << 32)) return SPECK_ERR_DIM_LIMIT;  // (the spans below stay inside 64 bits)
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (ldx < k || ldy < k) return SPECK_ERR_INVALID;
    // the plan was made from another shape: refused here; from another pattern of this shape: on the device
    if (A->rows != plan->rows || A->cols != plan->cols || A->nnz != plan->nnz) return SPECK_ERR_INVALID;
    if (A->rows && !A->row_offsets) return SPECK_ERR_INVALID;
    if (A->cols && k && !d_Y) return SPECK_ERR_INVALID;
    if (A->nnz && (!A->data || !A->col_ids || (k && !d_X))) return SPECK_ERR_INVALID;
    if ((d_X && is_one_of(d_X, A)) || (d_Y && is_one_of(d_Y, A))) return SPECK_ERR_INVALID;
    if (d_X && d_Y && A->rows && A->cols && k) {
        // what the call may touch: [d_X, d_X + (rows - 1) ldx + k) and [d_Y, d_Y + (cols - 1) ldy + k), padding inside included
        const u64 x0 = reinterpret_cast<uintptr_t>(d_X), y0 = reinterpret_cast<uintptr_t>(d_Y);
        const u64 xs = sizeof(B) * ((A->rows - 1) * ldx + k), ys = sizeof(B) * ((A->cols - 1) * ldy + k);
        if (x0 < y0 + ys && y0 < x0 + xs) return SPECK_ERR_INVALID;
    }
    if (info) *info = speck_spmm_t_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->cols == 0 || k == 0) return SPECK_OK;  // no row or no column of Y: nothing to write
    SpmmTStatus h{};
    const int rc = run_tile_call(cfg, spmm_t_scratch, kGuardNames, 3, " by the transposed product", [&](TileScratch* sc, hipStream_t s) {
        return spmm_t_run<T, B>(sc, s, plan, alpha, A, d_X, ldx, k, beta, d_Y, ldy, &h);
    });
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->cols_empty = h.rows_empty;
        info->cols_split = h.rows_split;
        info->tiles = tiles_touched(0, A->nnz);
        info->entries = A->nnz;
        info->terms = A->nnz * k;
    }
    return SPECK_OK;
}

}  // namespace

extern "C" {

int speck_spmm_t_f64(speck_config* cfg, const speck_tplan* plan, double alpha, const speck_dcsr* A, const double* d_X, uint64_t ldx,
                     uint32_t k, double beta, double* d_Y, uint64_t ldy, speck_spmm_t_info* info)
{
    return spmm_t_impl<double>(cfg, plan, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_t_f32(speck_config* cfg, const speck_tplan* plan, double alpha, const speck_dcsr* A, const double* d_X, uint64_t ldx,
                     uint32_t k, double beta, double* d_Y, uint64_t ldy, speck_spmm_t_info* info)
{
    return spmm_t_impl<float>(cfg, plan, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_t_f64_b32(speck_config* cfg, const speck_tplan* plan, double alpha, const speck_dcsr* A, const float* d_X, uint64_t ldx,
                         uint32_t k, double beta, float* d_Y, uint64_t ldy, speck_spmm_t_info* info)
{
    return spmm_t_impl<double>(cfg, plan, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_t_f32_b32(speck_config* cfg, const speck_tplan* plan, double alpha, const speck_dcsr* A, const float* d_X, uint64_t ldx,
                         uint32_t k, double beta, float* d_Y, uint64_t ldy, speck_spmm_t_info* info)
{
    return spmm_t_impl<float>(cfg, plan, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

}  // extern "C"
