// spmv.hip -- speck_spmv_*: y = alpha A x + beta y on a device CSR, x and y device vectors of doubles.  The walk of
// reduce.hip with the term a(i,j) x[j] in place of g(a(i,j)): the same entry tiles, the same combination tree
// (tile_combine.hpp), so y (alpha = 1, beta = 0) is bit for bit reduce(SUM) of scale(A, col = x).  The reference has no
// counterpart.
//
//   tile_check_kernel     (tile_combine.hpp) a thread per row: the offsets, the empty rows, the rows of every tile's first
//                         and last entry.  Raises `invalid` in the status block.
//   spmv_tile_kernel      queued behind it, looks at that verdict first.  A workgroup per ENTRY TILE; a thread takes its 16
//                         values and its 16 column ids (16-byte loads where both arrays lie on 16-byte boundaries and the
//                         tile is whole, entry by entry elsewhere), then issues the 16 gathers of x before the first is
//                         consumed.  An id >= cols raises `bad_id` and is NOT followed: the gather goes to the clamped id
//                         and its term is never used outside the scratch.  The segmented combine leaves the sum of every
//                         row that lies whole in the tile in the scratch array `sums`, the rest in the tile's record.
//   spmv_finish_kernel    queued last: it sees the verdict of EVERY tile, and only it writes y.  Three kinds of workgroups:
//                         a wave per tile finishes the row that leaves the tile open (the chain of the reduction) and
//                         writes its y; a thread per row writes the y of a row that lies in one tile (from `sums`) or
//                         holds no entry (+0.0); one workgroup counts the split rows.  Each row is written once by one
//                         thread, which reads y_i itself where beta != 0.
// Nothing of y before the verdict: the ids are checked by the tiles that read them, so the verdict is complete only
// when every tile has run; the sums wait in `sums` (16 rows bytes of traffic, against the 4 nnz bytes and the extra pass
// of a checking stream over col_ids in front, as scale.hip has one).  No floating-point atomic; one read-back, at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "entry_tiles.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "side_call.hpp"
#include "spmv.hpp"
#include "tile_combine.hpp"

// every product and every sum is rounded on its own: the terms are those of scale.hip, the sums those of reduce.hip
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SPMV_TILE_ENTRIES && kTile == SPECK_REDUCE_TILE_ENTRIES, "the reduction's tiles");
using Sum = Op<SPECK_REDUCE_SUM>;

struct SpmvStatus {
    u32 invalid;  // the offsets (tile_check_kernel)
    u32 base;     // row_offsets[0]
    unsigned long long rows_empty, rows_split;
    u32 bad_id;   // a column id >= cols (spmv_tile_kernel)
};

template <typename T>
struct SpmvArgs {
    const u32* ro;
    const u32* col;
    const T* data;
    const double* x;
    double* sums;  // rows doubles: s_i of the rows that lie whole in one tile
    u64 nnz;
    u32 rows, cols;  // cols >= 1
    u32 aligned;     // data and col start on 16-byte boundaries
    TileRec* recs;
    const u32* tile_rows;
    SpmvStatus* st;
};

template <typename V, u32 N>
struct alignas(16) Vec {
    V v[N];
};

// ------------------------------------------------------------------------------------------------ tiles
template <typename T>
__global__ __launch_bounds__(kThreads) void spmv_tile_kernel(const SpmvArgs<T> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    const u32 t = threadIdx.x;
    const u64 base = g.st->base, end = base + g.nnz;
    const u64 tile0 = (base / kTile + blockIdx.x) * kTile;
    if (tile0 >= end) return;  // (the grid is sized without knowing the base)
    const u64 lo = std::max(tile0, base), hi = std::min(tile0 + kTile, end);
    const bool whole = lo == tile0 && hi == tile0 + kTile;

    // the thread's 16 entries and their column ids; where the matrix does not reach: id 0, never used
    T a[kPer];
    u32 c[kPer];
    const u64 q0 = tile0 + u64(t) * kPer;
    if (whole && g.aligned) {
        constexpr u32 N = 16 / sizeof(T);
        const Vec<T, N>* src = reinterpret_cast<const Vec<T, N>*>(g.data + q0);
        const Vec<u32, 4>* cs = reinterpret_cast<const Vec<u32, 4>*>(g.col + q0);
        Vec<T, N> av[kPer / N];
        Vec<u32, 4> cv[kPer / 4];
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) av[k] = src[k];
#pragma unroll
        for (u32 k = 0; k < kPer / 4; ++k) cv[k] = cs[k];
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) a[k] = av[k / N].v[k % N], c[k] = cv[k / 4].v[k % 4];
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            const bool in = p >= lo && p < hi;
            a[k] = in ? g.data[p] : T(0);
            c[k] = in ? g.col[p] : 0u;
        }
    }

    // an id the matrix has no column for is reported and not followed; all 16 gathers are in flight before the first term
    const u32 last = g.cols - 1u;
    bool bad = false;
    double xv[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        bad |= c[k] > last;
        xv[k] = g.x[std::min(c[k], last)];
    }
    if (bad) g.st->bad_id = 1;
    double v[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        const u64 p = q0 + k;
        v[k] = (whole || (p >= lo && p < hi)) ? (double)a[k] * xv[k] : Sum::ident();
    }

    // (rows without entries and rows in more than one tile: spmv_finish_kernel)
    double* const sums = g.sums;
    combine_tile<Sum>(s_tile, v, g.ro, g.tile_rows, g.recs + blockIdx.x, tile0, lo, hi, [sums](u32 r, double val) { sums[r] = val; });
}

// ------------------------------------------------------------------------------------------------ finish, and y
__device__ __forceinline__ void write_y(double* __restrict__ y, u32 r, double s, double alpha, double beta)
{
#pragma clang fp contract(off)
    const double as = alpha * s;
    if (beta == 0.0) y[r] = as;  // (y is not read: what it held does not survive)
    else {
        const double by = beta * y[r];
        y[r] = as + by;
    }
}

__global__ __launch_bounds__(kThreads) void spmv_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 chain_blocks,
                                                               u32 row_blocks, const double* __restrict__ sums,
                                                               const TileRec* __restrict__ recs, double alpha, double beta,
                                                               double* __restrict__ y, SpmvStatus* st)
{
    SPECK_POISON();
    __shared__ double s_w[kWaves];
    __shared__ u32 s_split[kWaves];
    if (st->invalid || st->bad_id) return;  // (every tile has run: the verdict is complete, and nothing of y was written)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u64 base = st->base;
    const u32 ntiles = tiles_touched(base, nnz);
    if (blockIdx.x < chain_blocks) {
        u32 row;
        double val;
        if (chain_finish<Sum>(recs, blockIdx.x * kWaves + wid, ntiles, base / kTile, &row, &val) && lane == 0) write_y(y, row, val, alpha, beta);
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        const u32 r = (blockIdx.x - chain_blocks) * kThreads + t;
        if (r >= rows) return;
        const u32 b = ro[r], e = ro[r + 1];
        if (b == e) write_y(y, r, Sum::ident(), alpha, beta);
        else if (b / kTile == (e - 1u) / kTile) write_y(y, r, sums[r], alpha, beta);  // (else: the chain above)
    } else {
        double total;
        u32 split;
        if (totals_finish<Sum>(recs, ntiles, s_w, s_split, &total, &split)) st->rows_split = split;
    }
}

// ------------------------------------------------------------------------------------------------ host
bool on_16_bytes(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T>
int spmv_run(SpmvScratch* sc, hipStream_t s, double alpha, const speck_dcsr* A, const double* d_x, double beta, double* d_y,
             SpmvStatus* h)
{
    const u32 rows = (u32)A->rows;
    const u32 max_tiles = entry_tiles_at_most(A->nnz, kTile);
    static_assert(sizeof(SpmvStatus) <= 256, "status block");
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    const size_t rec_bytes = up256(size_t(std::max(max_tiles, 1u)) * sizeof(TileRec));
    rc = sc->var.ensure(rec_bytes + up256(size_t(std::max(max_tiles, 1u)) * 8));
    if (rc != SPECK_OK) return rc;
    rc = sc->sums.ensure(up256(size_t(rows) * 8));
    if (rc != SPECK_OK) return rc;
    SpmvStatus* st = static_cast<SpmvStatus*>(sc->fixed.p);
    TileRec* recs = static_cast<TileRec*>(sc->var.p);
    u32* tile_rows = reinterpret_cast<u32*>(static_cast<unsigned char*>(sc->var.p) + rec_bytes);
    double* sums = static_cast<double*>(sc->sums.p);

    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SpmvStatus), s));
    SPECK_LAUNCH(tile_check_kernel<SpmvStatus>, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0, s, A->row_offsets, rows,
                 A->nnz, max_tiles, tile_rows, st);
    if (max_tiles) {
        const SpmvArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), d_x, sums, A->nnz, rows, (u32)A->cols,
                            on_16_bytes(A->data) && on_16_bytes(A->col_ids) ? 1u : 0u, recs, tile_rows, st};
        SPECK_LAUNCH(spmv_tile_kernel<T>, dim3(max_tiles), dim3(kThreads), 0, s, g);
    }
    const u32 chain_blocks = (max_tiles + kWaves - 1) / kWaves, row_blocks = (rows + kThreads - 1) / kThreads;
    SPECK_LAUNCH(spmv_finish_kernel, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 chain_blocks, row_blocks, sums, recs, alpha, beta, d_y, st);
    // the ONE read-back of the call: the two verdicts, the counters
    rc = read_status(s, st, h);
    if (rc != SPECK_OK) return rc;
    return (h->invalid || h->bad_id) ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kGuardNames[3] = {"spmv status", "spmv tile records and rows", "spmv row sums"};

bool is_one_of(const void* v, const speck_dcsr* X) { return v == X->data || v == X->col_ids || v == X->row_offsets; }

template <typename T>
int spmv_impl(speck_config* cfg, double alpha, const speck_dcsr* A, const double* d_x, double beta, double* d_y, speck_spmv_info* info)
{
    if (!A || alpha != alpha || beta != beta) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (A->rows && (!A->row_offsets || !d_y)) return SPECK_ERR_INVALID;
    if (A->nnz && (!A->data || !A->col_ids || !d_x)) return SPECK_ERR_INVALID;
    // (entries without a row to hold them; entries without a column to point at: every id is >= cols)
    if (A->nnz && (A->rows == 0 || A->cols == 0)) return SPECK_ERR_INVALID;
    if ((d_x && is_one_of(d_x, A)) || (d_y && is_one_of(d_y, A))) return SPECK_ERR_INVALID;
    if (d_x && d_y && A->rows && A->cols) {
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(d_x), y0 = reinterpret_cast<uintptr_t>(d_y);
        if (x0 < y0 + 8 * A->rows && y0 < x0 + 8 * A->cols) return SPECK_ERR_INVALID;
    }
    if (info) *info = speck_spmv_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0) return SPECK_OK;  // no row: nothing to write
    SpmvScratch own;
    SpmvScratch* sc = cfg ? spmv_scratch(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    SpmvStatus h{};
    int rc = spmv_run<T>(sc, s, alpha, A, d_x, beta, d_y, &h);
    if (rc != SPECK_OK) (void)hipStreamSynchronize(s);
    const void* whole[] = {sc->fixed.p, sc->var.p, sc->sums.p};
    rc = guard_check_buffers(whole, kGuardNames, 3, s, " by the matrix-vector product", rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->rows_empty = h.rows_empty;
        info->rows_split = h.rows_split;
        info->tiles = A->nnz ? (u64(h.base) + A->nnz - 1) / kTile - u64(h.base) / kTile + 1 : 0;
        info->entries = A->nnz;
    }
    return SPECK_OK;
}

}  // namespace

extern "C" {

int speck_spmv_f64(speck_config* cfg, double alpha, const speck_dcsr* A, const double* d_x, double beta, double* d_y,
                   speck_spmv_info* info)
{
    return spmv_impl<double>(cfg, alpha, A, d_x, beta, d_y, info);
}

int speck_spmv_f32(speck_config* cfg, double alpha, const speck_dcsr* A, const double* d_x, double beta, double* d_y,
                   speck_spmv_info* info)
{
    return spmv_impl<float>(cfg, alpha, A, d_x, beta, d_y, info);
}

}  // extern "C"
