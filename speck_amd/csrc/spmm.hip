// spmm.hip -- speck_spmm_*: Y = alpha A X + beta Y on a device CSR, X (cols x k) and Y (rows x k) row-major device arrays of
// doubles with leading dimensions ldx, ldy.  The walk of spmv.hip with A read ONCE for all k columns: the same entry
// tiles, the same combination tree (tile_combine.hpp) per column, so column c of Y is bit for bit what speck_spmv_* writes
// for X(:,c) and Y(:,c).  The reference has no counterpart.
//
//   tile_check_kernel     (tile_combine.hpp) a thread per row: the offsets, the empty rows, the rows of every tile's first
//                         and last entry.  Raises `invalid` in the status block.
//   spmm_tile_kernel      queued behind it, looks at that verdict first.  A workgroup per ENTRY TILE; a thread takes its 16
//                         values and its 16 column ids ONCE (16-byte loads under spmv's condition, entry by entry
//                         elsewhere), checks and clamps the ids ONCE (an id >= cols raises `bad_id` and is NOT followed),
//                         builds the tile's row-start bitmap ONCE (tile_begin), then walks the k columns in blocks of
//                         kCB = 4: all 16 kCB gathers X[id ldx + c0 ..) of a block are issued before the first term
//                         -- one 16-byte load per entry and pair of columns where d_X lies on 16 bytes and ldx is even,
//                         8-byte loads elsewhere, the same bits -- then per column the terms and the segmented combine
//                         (combine_terms), with a barrier before the next column takes the LDS.  What k leaves over
//                         goes in a pair and alone.  A row whole in the tile leaves its sum in sums[r k + c], the rest
//                         in the record of (tile, column).  The 64 gathered doubles of a block put the kernel at 245
//                         registers and two waves per SIMD, not the four the LDS allows: measured against one column
//                         per round at 99 registers and four waves, and 1.4 to 2.9 times faster from k = 8 on where X
//                         does not stay in the cache.
//   spmm_finish_kernel    queued last: it sees the verdict of EVERY tile, and only it writes Y.  Three kinds of workgroups:
//                         a wave per (tile, column) finishes the row that leaves the tile open; a thread per (row, column),
//                         adjacent lanes on adjacent columns, writes a row that lies in one tile (from `sums`) or holds
//                         no entry (+0.0); one workgroup counts the split rows.  Every Y(i,c) is written once by one thread,
//                         which reads it itself where beta != 0.  The padding [k, ldy) of a row is neither read nor written.
// All index arithmetic i ld + c is 64-bit.  No floating-point atomic; one read-back, at the end.
// What is spmv.hip's word for word -- a tile kernel's opening, the load of the entries, the check of the ids, the write of
// a y; the scratch, the check's launch, the frame of the call -- is tile_combine.hpp's and tile_call.hpp's.
//
// speck_spmm_*_b32: X and Y in float (B = float below).  The same walk through the same functions; an element of X is
// widened where its term is formed ((double)a * (double)x: the widening is exact), Y is rounded to float once, in write_y.
// A 16-byte load holds FOUR columns of an entry: a block of kCB32 columns keeps 16 kCB32 floats in flight -- half the
// registers of the doubles' block -- loaded 16 bytes at a time where d_X lies on 16 bytes and ldx % 4 == 0, 8 bytes where
// d_X lies on 8 and ldx is even, 4 bytes elsewhere, with the same bits.  The kernels are the doubles' with the block type as a
// template parameter (a body shared through a function moved the doubles' registers: DESIGN.md 4.26).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "launch.hpp"
#include "tile_call.hpp"

// every product and every sum is rounded on its own: the terms and the sums are those of spmv.hip
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SPMV_TILE_ENTRIES, "spmv's tiles");
using Sum = Op<SPECK_REDUCE_SUM>;

// the columns whose gathers are in flight together (the registers: DESIGN.md 4.17)
constexpr u32 kCB = SPECK_SPMM_COLUMN_BLOCK;
static_assert(kCB % 2 == 0, "a 16-byte gather takes two columns");
// the same for float blocks (SPECK_SPMM_B32_FORCE_BLOCK: measurement builds only, profiles/blocks32.txt)
#ifdef SPECK_SPMM_B32_FORCE_BLOCK
constexpr u32 kCB32 = SPECK_SPMM_B32_FORCE_BLOCK;
#else
constexpr u32 kCB32 = SPECK_SPMM_COLUMN_BLOCK_B32;
#endif
static_assert(kCB32 % 4 == 0, "a 16-byte gather takes four columns");

template <typename T, typename B = double>
struct SpmmArgs {
    const u32* ro;
    const u32* col;
    const T* data;
    const B* x;
    double* sums;  // rows k doubles: s(i,c) of the rows that lie whole in one tile
    u64 nnz, ldx;
    u32 rows, cols;  // cols >= 1
    u32 k;           // >= 1
    u32 max_tiles;   // the records of column c start at recs + c max_tiles
    u32 aligned;     // data and col start on 16-byte boundaries
    u32 pairs;       // x starts on a 16-byte boundary and ldx is even: X(j, c) with even c lies on one (B = float: the
                     // elements of the widest load every X(j, c) with c a multiple of it is aligned to -- 4, 2 or 1)
    TileRec* recs;
    const u32* tile_rows;
    ProductStatus* st;
};

// ------------------------------------------------------------------------------------------------ tiles
// The columns [c0, c0 + W) of a tile whose row-start bitmap stands (tile_begin): all 16 W gathers X[id ldx + c0 ..) are
// issued before the first term, then per column the terms and the segmented combine, with a barrier before the next
// column takes the LDS.  VW: the elements of X a load takes -- X(j, c0) lies on a boundary of VW elements for every j and
// VW divides W (doubles: one 16-byte load per entry and pair of columns; floats: per four columns, or 8 bytes per pair).
// a: the thread's values, in double; c: its ids, checked, < cols; in_mask: which entries the matrix reaches.  A gathered
// element stays in B until its term is formed.
template <u32 W, u32 VW, typename T, typename B>
__device__ __forceinline__ void column_block(const SpmmArgs<T, B>& g, TileLds& s_tile, const TileRows rows, const double (&a)[kPer],
                                             u32 (&c)[kPer], u32 in_mask, const TileFrame& f, u32 c0)
{
#pragma clang fp contract(off)
    static_assert(W % VW == 0 && VW * sizeof(B) <= 16, "whole loads of at most 16 bytes");
    // (the ids pass through an empty asm: the 16 addresses derived from them -- 32 registers -- are then computed per
    //  block and not kept over the whole column loop)
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) asm volatile("" : "+v"(c[e]));
    B xv[W][kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) {
        const B* src = g.x + (u64(c[e]) * g.ldx + c0);
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
    double* const sums = g.sums;
    const u32 nk = g.k;
#pragma unroll
    for (u32 j = 0; j < W; ++j) {
        double v[kPer];
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) v[e] = ((in_mask >> e) & 1u) ? a[e] * (double)xv[j][e] : Sum::ident();
        const u32 cc = c0 + j;
        combine_terms<Sum>(s_tile, rows, v, g.ro, g.recs + (u64(cc) * g.max_tiles + blockIdx.x), f.tile0, f.lo, f.hi,
                           [sums, nk, cc](u32 r, double val) { sums[u64(r) * nk + cc] = val; });
        // the rows that end in the tile were read from val and incl: the next column overwrites both
        __syncthreads();
    }
}

template <typename T, typename B>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void spmm_tile_kernel(const SpmmArgs<T, B> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;

    // the thread's 16 entries (as doubles: the conversion is exact and happens once) and their column ids, once for all
    // columns; where the matrix does not reach: id 0, never used
    T at[kPer];
    double a[kPer];
    u32 c[kPer];
    load_entries<true>(f, f.whole && g.aligned, g.data, g.col, at, c);
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) a[e] = (double)at[e];

    // an id the matrix has no column for is reported and not followed: from here on c holds ids < cols only
    const u32 last = g.cols - 1u;
    bool bad = false;
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) c[e] = clamp_id(c[e], last, &bad);
    if (bad) g.st->bad_id = 1;
    // (the entries of a tile that is not whole which the matrix does not reach: their term is the identity)
    u32 in_mask = 0xFFFFu;
    if (!f.whole) {
        in_mask = 0;
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) in_mask |= u32(entry_in(f, e)) << e;
    }

    const TileRows rows = tile_begin(s_tile, g.ro, g.tile_rows, f.tile0);
    // the columns in blocks of kCB, then what is left in pairs and alone; one straight path per form of block
    const u32 nk = g.k;
    u32 c0 = 0;
    if constexpr (sizeof(B) == 8) {
        if (g.pairs) {
            for (; c0 + kCB <= nk; c0 += kCB) column_block<kCB, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
            for (; c0 + 2 <= nk; c0 += 2) column_block<2, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
        } else {
            for (; c0 + kCB <= nk; c0 += kCB) column_block<kCB, 1>(g, s_tile, rows, a, c, in_mask, f, c0);
        }
    } else {
        // (c0 stays a multiple of the load's width: blocks of kCB32, then four, then two columns)
        if (g.pairs == 4) {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 4>(g, s_tile, rows, a, c, in_mask, f, c0);
            if constexpr (kCB32 > 4)
                for (; c0 + 4 <= nk; c0 += 4) column_block<4, 4>(g, s_tile, rows, a, c, in_mask, f, c0);
        } else if (g.pairs == 2) {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
        } else {
            for (; c0 + kCB32 <= nk; c0 += kCB32) column_block<kCB32, 1>(g, s_tile, rows, a, c, in_mask, f, c0);
        }
        if (g.pairs >= 2)
            for (; c0 + 2 <= nk; c0 += 2) column_block<2, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
    }
    for (; c0 < nk; ++c0) column_block<1, 1>(g, s_tile, rows, a, c, in_mask, f, c0);
}

// ------------------------------------------------------------------------------------------------ finish, and Y
template <typename B>
__global__ __launch_bounds__(kThreads) void spmm_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 k, u32 max_tiles,
                                                               u32 chain_blocks, u32 row_blocks, const double* __restrict__ sums,
                                                               const TileRec* __restrict__ recs, double alpha, double beta,
                                                               B* __restrict__ y, u64 ldy, ProductStatus* st)
{
    SPECK_POISON();
    __shared__ double s_w[kWaves];
    __shared__ u32 s_split[kWaves];
    if (st->invalid || st->bad_id) return;  // (every tile has run: the verdict is complete, and nothing of Y was written)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u64 base = st->base;
    const u32 ntiles = tiles_touched(base, nnz);
    if (blockIdx.x < chain_blocks) {
        // a wave per (tile, column), the tiles of a column side by side
        const u64 w = u64(blockIdx.x) * kWaves + wid;
        const u32 c = (u32)(w / max_tiles), i = (u32)(w - u64(c) * max_tiles);
        u32 row;
        double val;
        if (c < k && chain_finish<Sum>(recs + u64(c) * max_tiles, i, ntiles, base / kTile, &row, &val) && lane == 0)
            write_y(y, u64(row) * ldy + c, val, alpha, beta);
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        // a thread per (row, column), adjacent lanes on adjacent columns: (r, c) = divmod(256 block + t, k), the 64-bit
        // division once per workgroup
        const u64 first = u64(blockIdx.x - chain_blocks) * kThreads;
        const u64 r0 = first / k;
        const u32 in = (u32)(first - r0 * k) + t;  // < k + 256
        const u64 r64 = r0 + in / k;
        const u32 c = in % k;
        if (r64 >= rows) return;
        const u32 r = (u32)r64;
        const u32 b = ro[r], e = ro[r + 1];
        if (b == e) write_y(y, u64(r) * ldy + c, Sum::ident(), alpha, beta);
        else if (b / kTile == (e - 1u) / kTile) write_y(y, u64(r) * ldy + c, sums[u64(r) * k + c], alpha, beta);  // (else: the chain above)
    } else {
        // (which rows are split is a matter of A alone: column 0's records tell)
        double total;
        u32 split;
        if (totals_finish<Sum>(recs, ntiles, s_w, s_split, &total, &split)) st->rows_split = split;
    }
}

// ------------------------------------------------------------------------------------------------ host
// the widest load every X(j, c) with c a multiple of its width is aligned to, as SpmmArgs::pairs has it
inline u32 gather_width(const double* d_X, u64 ldx) { return on_16_bytes(d_X) && ldx % 2 == 0 ? 1u : 0u; }
inline u32 gather_width(const float* d_X, u64 ldx)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(d_X);
    return at % 16 == 0 && ldx % 4 == 0 ? 4u : at % 8 == 0 && ldx % 2 == 0 ? 2u : 1u;
}

template <typename T, typename B>
int spmm_run(TileScratch* sc, hipStream_t s, double alpha, const speck_dcsr* A, const B* d_X, u64 ldx, u32 k, double beta,
             B* d_Y, u64 ldy, ProductStatus* h)
{
    const u32 rows = (u32)A->rows;
    TileWork<ProductStatus> w;
    int rc = carve_and_check(sc, s, A, k, size_t(rows) * k, &w);
    if (rc != SPECK_OK) return rc;
    if (w.max_tiles) {
        const SpmmArgs<T, B> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), d_X, w.sums, A->nnz, ldx, rows, (u32)A->cols, k,
                               w.max_tiles, on_16_bytes(A->data) && on_16_bytes(A->col_ids) ? 1u : 0u, gather_width(d_X, ldx), w.recs,
                               w.tile_rows, w.st};
        SPECK_LAUNCH((spmm_tile_kernel<T, B>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
    }
    // (rows <= 2^27, k <= 2^10, tiles <= 2^20 + 1: the grid stays below 2^30)
    const u32 chain_blocks = (u32)((u64(w.max_tiles) * k + kWaves - 1) / kWaves);
    const u32 row_blocks = (u32)((u64(rows) * k + kThreads - 1) / kThreads);
    SPECK_LAUNCH(spmm_finish_kernel<B>, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz, k,
                 w.max_tiles, chain_blocks, row_blocks, w.sums, w.recs, alpha, beta, d_Y, ldy, w.st);
    // the ONE read-back of the call: the two verdicts, the counters
    rc = read_status(s, w.st, h);
    if (rc != SPECK_OK) return rc;
    return (h->invalid || h->bad_id) ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kGuardNames[3] = {"spmm status", "spmm tile records and rows", "spmm row sums"};

template <typename T, typename B>
int spmm_impl(speck_config* cfg, double alpha, const speck_dcsr* A, const B* d_X, u64 ldx, u32 k, double beta, B* d_Y,
              u64 ldy, speck_spmm_info* info)
{
    if (!A || alpha != alpha || beta != beta) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || k > SPECK_SPMM_MAX_RHS) return SPECK_ERR_DIM_LIMIT;
    if (ldx > (1ull << 32) || ldy > (1ull << 32)) return SPECK_ERR_DIM_LIMIT;  // (the spans below stay inside 64 bits)
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (ldx < k || ldy < k) return SPECK_ERR_INVALID;
    if (A->rows && (!A->row_offsets || (k && !d_Y))) return SPECK_ERR_INVALID;
    if (A->nnz && (!A->data || !A->col_ids || (k && !d_X))) return SPECK_ERR_INVALID;
    // (entries without a row to hold them; entries without a column to point at: every id is >= cols)
    if (A->nnz && (A->rows == 0 || A->cols == 0)) return SPECK_ERR_INVALID;
    if ((d_X && is_one_of(d_X, A)) || (d_Y && is_one_of(d_Y, A))) return SPECK_ERR_INVALID;
    if (d_X && d_Y && A->rows && A->cols && k) {
        // what the call may touch: [d_X, d_X + (cols - 1) ldx + k) and [d_Y, d_Y + (rows - 1) ldy + k), padding inside included
        const u64 x0 = reinterpret_cast<uintptr_t>(d_X), y0 = reinterpret_cast<uintptr_t>(d_Y);
        const u64 xs = sizeof(B) * ((A->cols - 1) * ldx + k), ys = sizeof(B) * ((A->rows - 1) * ldy + k);
        if (x0 < y0 + ys && y0 < x0 + xs) return SPECK_ERR_INVALID;
    }
    if (info) *info = speck_spmm_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0 || k == 0) return SPECK_OK;  // no row or no column: nothing to write
    ProductStatus h{};
    const int rc = run_tile_call(cfg, spmm_scratch, kGuardNames, 3, " by the product with several right-hand sides",
                                 [&](TileScratch* sc, hipStream_t s) { return spmm_run<T, B>(sc, s, alpha, A, d_X, ldx, k, beta, d_Y, ldy, &h); });
    if (rc != SPECK_OK) return rc;
    if (info) {
        fill_tile_info(info, h, A);
        info->terms = A->nnz * k;
    }
    return SPECK_OK;
}

}  // namespace

extern "C" {

int speck_spmm_f64(speck_config* cfg, double alpha, const speck_dcsr* A, const double* d_X, uint64_t ldx, uint32_t k, double beta,
                   double* d_Y, uint64_t ldy, speck_spmm_info* info)
{
    return spmm_impl<double>(cfg, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_f32(speck_config* cfg, double alpha, const speck_dcsr* A, const double* d_X, uint64_t ldx, uint32_t k, double beta,
                   double* d_Y, uint64_t ldy, speck_spmm_info* info)
{
    return spmm_impl<float>(cfg, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_f64_b32(speck_config* cfg, double alpha, const speck_dcsr* A, const float* d_X, uint64_t ldx, uint32_t k, double beta,
                       float* d_Y, uint64_t ldy, speck_spmm_info* info)
{
    return spmm_impl<double>(cfg, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

int speck_spmm_f32_b32(speck_config* cfg, double alpha, const speck_dcsr* A, const float* d_X, uint64_t ldx, uint32_t k, double beta,
                       float* d_Y, uint64_t ldy, speck_spmm_info* info)
{
    return spmm_impl<float>(cfg, alpha, A, d_X, ldx, k, beta, d_Y, ldy, info);
}

}  // extern "C"
