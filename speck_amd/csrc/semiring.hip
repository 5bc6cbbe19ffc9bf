// semiring.hip -- speck_spmv_sr_* / speck_spmm_sr_*: y = [z (+)] A (x) x over a (min | max, + | x | second) semiring on a
// device CSR, vectors and row-major blocks of doubles.  The walk of spmv.hip and spmm.hip with the monoid Op<MIN> / Op<MAX>
// of tile_combine.hpp in place of Op<SUM>, the term a + x[j], a x[j] or x[j] alone in place of a x[j], and z (+) s in
// place of alpha s + beta y: the same entry tiles, the same records, the same chain.  min and max are exact, so the
// result does not depend on the order of the combination: equal to numpy's minimum / maximum.reduceat in value, NaN
// where that has a NaN.  The reference has no counterpart.
//
//   tile_check_kernel     (tile_combine.hpp) a thread per row: the offsets, the empty rows, the rows of every tile's first
//                         and last entry.  Raises `invalid` in the status block.
//   spmv_sr_tile_kernel   spmv_tile_kernel's walk: a workgroup per ENTRY TILE, a thread takes its 16 values and ids (SECOND:
//                         the ids alone, load_ids -- A->data is never dereferenced), issues the 16 gathers of x through
//                         the clamped ids (an id >= cols raises `bad_id` and is NOT followed), forms the terms and leaves
//                         a row whole in the tile in `sums`, the rest in the tile's record.
//   spmm_sr_tile_kernel   spmm_tile_kernel's walk: entries, ids, check and row-start bitmap ONCE, then the k columns in
//                         blocks of SPECK_SPMM_COLUMN_BLOCK with all 16 x 4 gathers in flight (16-byte loads where d_X
//                         lies on 16 bytes and ldx is even), a pair and a single column for what k leaves over.
//   sr_finish_kernel      queued last, for both: it sees the verdict of EVERY tile, and only it writes y.  A wave per (tile,
//                         column) finishes the row that leaves the tile open; a thread per (row, column) writes a row that
//                         lies in one tile or holds no entry (the identity); one workgroup counts the split rows.  Every
//                         y(i,c) is written once by one thread, which reads z(i,c) itself first -- so z may BE y -- and
//                         tells whether the two differ; the workgroup adds that up in integers (block_counter_to) into
//                         `changed` of the status block.  A vector is a block with k = 1 and ld = 1.
// The kernels stand in a file of their own and spmv.hip / spmm.hip are untouched: their kernels keep their registers by
// construction (4.26 records what a shared body did to them once).
// Resources (gfx950, -O3; DESIGN.md 4.27 has the table): spmv_sr_tile_kernel 96 VGPRs with double values, 80 with float, 64
// with SECOND -- spmv_tile_kernel's 96 / 80 -- and 37456 bytes of LDS: 4 waves per SIMD, by the LDS; spmm_sr_tile_kernel 233
// VGPRs (SECOND: 201), the same LDS, pinned to 2 waves per SIMD as spmm_tile_kernel is; sr_finish_kernel 18 (a vector) and
// 20 VGPRs, 24 bytes of LDS, 8 waves per SIMD.  No scratch anywhere.
// All index arithmetic i ld + c is 64-bit.  No floating-point atomic; one read-back, at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "launch.hpp"
#include "tile_call.hpp"

// every term is rounded on its own: a + x[j] and a x[j] are one operation each
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SPMV_TILE_ENTRIES, "spmv's tiles");
constexpr u32 kCB = SPECK_SPMM_COLUMN_BLOCK;
static_assert(kCB % 2 == 0, "a 16-byte gather takes two columns");

// (x) of a semiring: SPECK_SR_* >> 1; (+) is SPECK_REDUCE_MIN where SPECK_SR_* is even, SPECK_REDUCE_MAX where odd
enum : int { kPlus = 0, kTimes = 1, kSecond = 2 };
static_assert((SPECK_SR_MIN_PLUS >> 1) == kPlus && (SPECK_SR_MAX_PLUS >> 1) == kPlus && (SPECK_SR_MIN_TIMES >> 1) == kTimes &&
                  (SPECK_SR_MAX_TIMES >> 1) == kTimes && (SPECK_SR_MIN_SECOND >> 1) == kSecond && (SPECK_SR_MAX_SECOND >> 1) == kSecond &&
                  !(SPECK_SR_MIN_PLUS & 1) && !(SPECK_SR_MIN_TIMES & 1) && !(SPECK_SR_MIN_SECOND & 1) && SPECK_SR_MAX_SECOND == 5,
              "how a semiring's number is taken apart");

template <int MUL>
__device__ __forceinline__ double sr_term(double a, double x)
{
#pragma clang fp contract(off)
    return MUL == kPlus ? a + x : MUL == kTimes ? a * x : x;
}

// the status block: tile_check_kernel's prefix, ProductStatus's bad_id, and the elements of y that differ from z
struct SemiringStatus {
    u32 invalid;
    u32 base;
    unsigned long long rows_empty, rows_split;
    u32 bad_id;
    u32 pad_;
    unsigned long long changed;
};

template <typename T>
struct SrArgs {
    const u32* ro;
    const u32* col;
    const T* data;  // not read with SECOND
    const double* x;
    double* sums;  // rows k doubles: s(i,c) of the rows that lie whole in one tile
    u64 nnz, ldx;
    u32 rows, cols;  // cols >= 1
    u32 k;           // >= 1
    u32 max_tiles;   // the records of column c start at recs + c max_tiles
    u32 aligned;     // col -- and data, where it is read -- start on 16-byte boundaries
    u32 pairs;       // x starts on a 16-byte boundary and ldx is even
    TileRec* recs;
    const u32* tile_rows;
    SemiringStatus* st;
};

// ------------------------------------------------------------------------------------------------ tiles, a vector
template <int MONO, int MUL, typename T>
__global__ __launch_bounds__(kThreads) void spmv_sr_tile_kernel(const SrArgs<T> g)
{
    using O = Op<MONO>;
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;

    T a[kPer];
    u32 c[kPer];
    if constexpr (MUL == kSecond) load_ids(f, f.whole && g.aligned, g.col, c);
    else load_entries<true>(f, f.whole && g.aligned, g.data, g.col, a, c);

    // an id the matrix has no column for is reported and not followed; all 16 gathers are in flight before the first term
    const u32 last = g.cols - 1u;
    bool bad = false;
    double xv[kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) xv[e] = g.x[clamp_id(c[e], last, &bad)];
    if (bad) g.st->bad_id = 1;
    double v[kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) {
        double t;
        if constexpr (MUL == kSecond) t = xv[e];
        else t = sr_term<MUL>((double)a[e], xv[e]);
        v[e] = (f.whole || entry_in(f, e)) ? t : O::ident();
    }

    double* const sums = g.sums;
    combine_tile<O>(s_tile, v, g.ro, g.tile_rows, g.recs + blockIdx.x, f.tile0, f.lo, f.hi, [sums](u32 r, double val) { sums[r] = val; });
}

// ------------------------------------------------------------------------------------------------ tiles, a block
// spmm.hip's column_block with the semiring's term and monoid: the columns [c0, c0 + W) of a tile whose row-start bitmap
// stands, all 16 W gathers issued before the first term; VW = 2: one 16-byte load per entry and pair of columns.
template <int MONO, int MUL, u32 W, u32 VW, typename T>
__device__ __forceinline__ void sr_column_block(const SrArgs<T>& g, TileLds& s_tile, const TileRows rows, const double (&a)[kPer],
                                                u32 (&c)[kPer], u32 in_mask, const TileFrame& f, u32 c0)
{
#pragma clang fp contract(off)
    using O = Op<MONO>;
    static_assert(W % VW == 0 && VW <= 2, "whole loads of at most 16 bytes");
    // (as in spmm.hip: the 16 addresses are computed per block and not kept over the whole column loop)
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) asm volatile("" : "+v"(c[e]));
    double xv[W][kPer];
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) {
        const double* src = g.x + (u64(c[e]) * g.ldx + c0);
        if (VW > 1) {
#pragma unroll
            for (u32 j = 0; j < W; j += VW) {
                const BlockVec<double, VW> p = reinterpret_cast<const BlockVec<double, VW>*>(src)[j / VW];
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
        for (u32 e = 0; e < kPer; ++e) {
            double t;
            if constexpr (MUL == kSecond) t = xv[j][e];
            else t = sr_term<MUL>(a[e], xv[j][e]);
            v[e] = ((in_mask >> e) & 1u) ? t : O::ident();
        }
        const u32 cc = c0 + j;
        combine_terms<O>(s_tile, rows, v, g.ro, g.recs + (u64(cc) * g.max_tiles + blockIdx.x), f.tile0, f.lo, f.hi,
                         [sums, nk, cc](u32 r, double val) { sums[u64(r) * nk + cc] = val; });
        // the rows that end in the tile were read from val and incl: the next column overwrites both
        __syncthreads();
    }
}

template <int MONO, int MUL, typename T>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void spmm_sr_tile_kernel(const SrArgs<T> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;

    // the thread's 16 entries (as doubles, converted once; SECOND: none) and their column ids, once for all columns
    double a[kPer];
    u32 c[kPer];
    if constexpr (MUL == kSecond) {
        load_ids(f, f.whole && g.aligned, g.col, c);
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) a[e] = 0.0;  // (never used)
    } else {
        T at[kPer];
        load_entries<true>(f, f.whole && g.aligned, g.data, g.col, at, c);
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) a[e] = (double)at[e];
    }

    // an id the matrix has no column for is reported and not followed: from here on c holds ids < cols only
    const u32 last = g.cols - 1u;
    bool bad = false;
#pragma unroll
    for (u32 e = 0; e < kPer; ++e) c[e] = clamp_id(c[e], last, &bad);
    if (bad) g.st->bad_id = 1;
    u32 in_mask = 0xFFFFu;
    if (!f.whole) {
        in_mask = 0;
#pragma unroll
        for (u32 e = 0; e < kPer; ++e) in_mask |= u32(entry_in(f, e)) << e;
    }

    const TileRows rows = tile_begin(s_tile, g.ro, g.tile_rows, f.tile0);
    const u32 nk = g.k;
    u32 c0 = 0;
    if (g.pairs) {
        for (; c0 + kCB <= nk; c0 += kCB) sr_column_block<MONO, MUL, kCB, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
        for (; c0 + 2 <= nk; c0 += 2) sr_column_block<MONO, MUL, 2, 2>(g, s_tile, rows, a, c, in_mask, f, c0);
    } else {
        for (; c0 + kCB <= nk; c0 += kCB) sr_column_block<MONO, MUL, kCB, 1>(g, s_tile, rows, a, c, in_mask, f, c0);
    }
    for (; c0 < nk; ++c0) sr_column_block<MONO, MUL, 1, 1>(g, s_tile, rows, a, c, in_mask, f, c0);
}

// ------------------------------------------------------------------------------------------------ finish, and y
// y[at] = s, or z[zat] (+) s: z is read before y is written, by the thread that writes -- z may be y.  Returns whether
// what was written differs from what z held (a NaN equals a NaN, +0.0 equals -0.0); 0 without a z.
template <typename O>
__device__ __forceinline__ u32 write_sr(double* y, u64 at, const double* z, u64 zat, double s)
{
    if (!z) {
        y[at] = s;
        return 0u;
    }
    const double zo = z[zat];
    const double yn = O::comb(zo, s);
    y[at] = yn;
    return (yn == zo || (yn != yn && zo != zo)) ? 0u : 1u;
}

template <int MONO, bool VECTOR>
__global__ __launch_bounds__(kThreads) void sr_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 k, u32 max_tiles,
                                                             u32 chain_blocks, u32 row_blocks, const double* __restrict__ sums,
                                                             const TileRec* __restrict__ recs, const double* z, u64 ldz, double* y,
                                                             u64 ldy, SemiringStatus* st)
{
    using O = Op<MONO>;
    SPECK_POISON();
    __shared__ double s_w[kWaves];
    __shared__ u32 s_split[kWaves];
    __shared__ unsigned long long s_changed;
    if (st->invalid || st->bad_id) return;  // (every tile has run: the verdict is complete, and nothing of y was written)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    if (t == 0) s_changed = 0;
    __syncthreads();
    const u64 base = st->base;
    const u32 ntiles = tiles_touched(base, nnz);
    u32 diff = 0;
    if (blockIdx.x < chain_blocks) {
        // a wave per (tile, column), the tiles of a column side by side
        const u64 w = u64(blockIdx.x) * kWaves + wid;
        const u32 c = VECTOR ? 0u : (u32)(w / max_tiles), i = (u32)(w - u64(c) * max_tiles);
        u32 row;
        double val;
        if (c < k && chain_finish<O>(recs + u64(c) * max_tiles, i, ntiles, base / kTile, &row, &val) && lane == 0)
            diff = write_sr<O>(y, u64(row) * ldy + c, z, u64(row) * ldz + c, val);
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        // a thread per (row, column), adjacent lanes on adjacent columns: (r, c) = divmod(256 block + t, k)
        // (VECTOR: k = 1 and every ld 1 -- a thread per row, no division)
        const u64 first = u64(blockIdx.x - chain_blocks) * kThreads;
        const u64 r0 = VECTOR ? first : first / k;
        const u32 in = (u32)(first - r0 * k) + t;  // < k + 256
        const u64 r64 = VECTOR ? first + t : r0 + in / k;
        const u32 c = VECTOR ? 0u : in % k;
        if (r64 < rows) {
            const u32 r = (u32)r64;
            const u32 b = ro[r], e = ro[r + 1];
            if (b == e) diff = write_sr<O>(y, u64(r) * ldy + c, z, u64(r) * ldz + c, O::ident());
            else if (b / kTile == (e - 1u) / kTile) diff = write_sr<O>(y, u64(r) * ldy + c, z, u64(r) * ldz + c, sums[u64(r) * k + c]);
            // (else: the chain above)
        }
    } else {
        // (which rows are split is a matter of A alone: column 0's records tell)
        double total;
        u32 split;
        if (totals_finish<O>(recs, ntiles, s_w, s_split, &total, &split)) st->rows_split = split;
    }
    block_counter_to(&st->changed, diff, &s_changed);
}

// ------------------------------------------------------------------------------------------------ host
template <int N>
using Int = std::integral_constant<int, N>;

// f(monoid, multiply) with the two as types; the semiring was checked
template <typename F>
int with_semiring(int semiring, F&& f)
{
    switch (semiring) {
        case SPECK_SR_MIN_PLUS: return f(Int<SPECK_REDUCE_MIN>{}, Int<kPlus>{});
        case SPECK_SR_MAX_PLUS: return f(Int<SPECK_REDUCE_MAX>{}, Int<kPlus>{});
        case SPECK_SR_MIN_TIMES: return f(Int<SPECK_REDUCE_MIN>{}, Int<kTimes>{});
        case SPECK_SR_MAX_TIMES: return f(Int<SPECK_REDUCE_MAX>{}, Int<kTimes>{});
        case SPECK_SR_MIN_SECOND: return f(Int<SPECK_REDUCE_MIN>{}, Int<kSecond>{});
        default: return f(Int<SPECK_REDUCE_MAX>{}, Int<kSecond>{});
    }
}

inline bool is_second(int semiring) { return (semiring >> 1) == kSecond; }

// vector: speck_spmv_sr_* (k = 1, every ld 1: spmv's tile kernel); otherwise speck_spmm_sr_*
template <typename T>
int sr_run(TileScratch* sc, hipStream_t s, bool vector, int semiring, const speck_dcsr* A, const double* d_X, u64 ldx, u32 k,
           const double* d_Z, u64 ldz, double* d_Y, u64 ldy, SemiringStatus* h)
{
    const u32 rows = (u32)A->rows;
    TileWork<SemiringStatus> w;
    int rc = carve_and_check(sc, s, A, k, size_t(rows) * k, &w);
    if (rc != SPECK_OK) return rc;
    if (w.max_tiles) {
        const bool aligned = on_16_bytes(A->col_ids) && (is_second(semiring) || on_16_bytes(A->data));
        const SrArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), d_X, w.sums, A->nnz, ldx, rows, (u32)A->cols, k,
                          w.max_tiles, aligned ? 1u : 0u, on_16_bytes(d_X) && ldx % 2 == 0 ? 1u : 0u, w.recs, w.tile_rows, w.st};
        rc = with_semiring(semiring, [&](auto mono, auto mul) {
            constexpr int MONO = decltype(mono)::value, MUL = decltype(mul)::value;
            if (vector) SPECK_LAUNCH((spmv_sr_tile_kernel<MONO, MUL, T>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
            else SPECK_LAUNCH((spmm_sr_tile_kernel<MONO, MUL, T>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
            return SPECK_OK;
        });
        if (rc != SPECK_OK) return rc;
    }
    // (rows <= 2^27, k <= 2^10, tiles <= 2^20 + 1: the grid stays below 2^30)
    const u32 chain_blocks = (u32)((u64(w.max_tiles) * k + kWaves - 1) / kWaves);
    const u32 row_blocks = (u32)((u64(rows) * k + kThreads - 1) / kThreads);
    const auto finish = [&](auto kernel) {
        SPECK_LAUNCH(kernel, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz, k, w.max_tiles,
                     chain_blocks, row_blocks, w.sums, w.recs, d_Z, ldz, d_Y, ldy, w.st);
    };
    if (semiring & 1) vector ? finish(sr_finish_kernel<SPECK_REDUCE_MAX, true>) : finish(sr_finish_kernel<SPECK_REDUCE_MAX, false>);
    else vector ? finish(sr_finish_kernel<SPECK_REDUCE_MIN, true>) : finish(sr_finish_kernel<SPECK_REDUCE_MIN, false>);
    // the ONE read-back of the call: the two verdicts, the counters
    rc = read_status(s, w.st, h);
    if (rc != SPECK_OK) return rc;
    return (h->invalid || h->bad_id) ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kVecGuardNames[3] = {"spmv_sr status", "spmv_sr tile records and rows", "spmv_sr row results"};
const char* const kBlockGuardNames[3] = {"spmm_sr status", "spmm_sr tile records and rows", "spmm_sr row results"};

template <typename T>
int sr_impl(speck_config* cfg, bool vector, int semiring, const speck_dcsr* A, const double* d_X, u64 ldx, u32 k, const double* d_Z,
            u64 ldz, double* d_Y, u64 ldy, speck_semiring_info* info)
{
    if (!A || semiring < SPECK_SR_MIN_PLUS || semiring > SPECK_SR_MAX_SECOND) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || k > SPECK_SPMM_MAX_RHS) return SPECK_ERR_DIM_LIMIT;
    if (ldx > (1ull << 32) || ldy > (1ull << 32) || (d_Z && ldz > (1ull << 32))) return SPECK_ERR_DIM_LIMIT;  // (the spans stay inside 64 bits)
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (ldx < k || ldy < k || (d_Z && ldz < k)) return SPECK_ERR_INVALID;
    if (A->rows && (!A->row_offsets || (k && !d_Y))) return SPECK_ERR_INVALID;
    if (A->nnz && (!A->col_ids || (k && !d_X) || (!is_second(semiring) && !A->data))) return SPECK_ERR_INVALID;
    // (entries without a row to hold them; entries without a column to point at: every id is >= cols)
    if (A->nnz && (A->rows == 0 || A->cols == 0)) return SPECK_ERR_INVALID;
    if ((d_X && is_one_of(d_X, A)) || (d_Y && is_one_of(d_Y, A)) || (d_Z && is_one_of(d_Z, A))) return SPECK_ERR_INVALID;
    if (d_Y && A->rows && k) {
        // what the call may touch: [d_X, d_X + (cols - 1) ldx + k), [d_Y, d_Y + (rows - 1) ldy + k) and the same of Z with
        // ldz, padding inside included.  Y may share no byte with X; with Z none, or all: the same pointer and the same ld
        const u64 y0 = reinterpret_cast<uintptr_t>(d_Y), ys = 8 * ((A->rows - 1) * ldy + k);
        if (d_X && A->cols) {
            const u64 x0 = reinterpret_cast<uintptr_t>(d_X), xs = 8 * ((A->cols - 1) * ldx + k);
            if (x0 < y0 + ys && y0 < x0 + xs) return SPECK_ERR_INVALID;
        }
        if (d_Z) {
            const u64 z0 = reinterpret_cast<uintptr_t>(d_Z), zs = 8 * ((A->rows - 1) * ldz + k);
            if (z0 == y0 ? ldz != ldy : (z0 < y0 + ys && y0 < z0 + zs)) return SPECK_ERR_INVALID;
        }
    }
    if (info) *info = speck_semiring_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0 || k == 0) return SPECK_OK;  // no row or no column: nothing to write
    SemiringStatus h{};
    const int rc = run_tile_call(cfg, vector ? spmv_sr_scratch : spmm_sr_scratch, vector ? kVecGuardNames : kBlockGuardNames, 3,
                                 " by the semiring product", [&](TileScratch* sc, hipStream_t s) {
                                     return sr_run<T>(sc, s, vector, semiring, A, d_X, ldx, k, d_Z, ldz, d_Y, ldy, &h);
                                 });
    if (rc != SPECK_OK) return rc;
    if (info) {
        fill_tile_info(info, h, A);
        info->terms = A->nnz * k;
        info->changed = h.changed;
    }
    return SPECK_OK;
}

}  // namespace

extern "C" {

int speck_spmv_sr_f64(speck_config* cfg, int semiring, const speck_dcsr* A, const double* d_x, const double* d_z, double* d_y,
                      speck_semiring_info* info)
{
    return sr_impl<double>(cfg, true, semiring, A, d_x, 1, 1, d_z, 1, d_y, 1, info);
}

int speck_spmv_sr_f32(speck_config* cfg, int semiring, const speck_dcsr* A, const double* d_x, const double* d_z, double* d_y,
                      speck_semiring_info* info)
{
    return sr_impl<float>(cfg, true, semiring, A, d_x, 1, 1, d_z, 1, d_y, 1, info);
}

int speck_spmm_sr_f64(speck_config* cfg, int semiring, const speck_dcsr* A, const double* d_X, uint64_t ldx, uint32_t k,
                      const double* d_Z, uint64_t ldz, double* d_Y, uint64_t ldy, speck_semiring_info* info)
{
    return sr_impl<double>(cfg, false, semiring, A, d_X, ldx, k, d_Z, ldz, d_Y, ldy, info);
}

int speck_spmm_sr_f32(speck_config* cfg, int semiring, const speck_dcsr* A, const double* d_X, uint64_t ldx, uint32_t k,
                      const double* d_Z, uint64_t ldz, double* d_Y, uint64_t ldy, speck_semiring_info* info)
{
    return sr_impl<float>(cfg, false, semiring, A, d_X, ldx, k, d_Z, ldz, d_Y, ldy, info);
}

}  // extern "C"
