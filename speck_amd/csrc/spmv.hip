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
// A tile kernel's opening, the load of the entries, the check of the ids and the write of a y are tile_combine.hpp's; the
// scratch, the check's launch and the frame of the call tile_call.hpp's: spmm.hip stands on the same.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "launch.hpp"
#include "tile_call.hpp"

// every product and every sum is rounded on its own: the terms are those of scale.hip, the sums those of reduce.hip
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;
static_assert(kTile == SPECK_SPMV_TILE_ENTRIES && kTile == SPECK_REDUCE_TILE_ENTRIES, "the reduction's tiles");
using Sum = Op<SPECK_REDUCE_SUM>;

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
    ProductStatus* st;
};

// ------------------------------------------------------------------------------------------------ tiles
template <typename T>
__global__ __launch_bounds__(kThreads) void spmv_tile_kernel(const SpmvArgs<T> g)
{
    SPECK_POISON();
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;

    // the thread's 16 entries and their column ids; where the matrix does not reach: id 0, never used
    T a[kPer];
    u32 c[kPer];
    load_entries<true>(f, f.whole && g.aligned, g.data, g.col, a, c);

    // an id the matrix has no column for is reported and not followed; all 16 gathers are in flight before the first term
    const u32 last = g.cols - 1u;
    bool bad = false;
    double xv[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) xv[k] = g.x[clamp_id(c[k], last, &bad)];
    if (bad) g.st->bad_id = 1;
    double v[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) v[k] = (f.whole || entry_in(f, k)) ? (double)a[k] * xv[k] : Sum::ident();

    // (rows without entries and rows in more than one tile: spmv_finish_kernel)
    double* const sums = g.sums;
    combine_tile<Sum>(s_tile, v, g.ro, g.tile_rows, g.recs + blockIdx.x, f.tile0, f.lo, f.hi, [sums](u32 r, double val) { sums[r] = val; });
}

// ------------------------------------------------------------------------------------------------ finish, and y
__global__ __launch_bounds__(kThreads) void spmv_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 chain_blocks,
                                                               u32 row_blocks, const double* __restrict__ sums,
                                                               const TileRec* __restrict__ recs, double alpha, double beta,
                                                               double* __restrict__ y, ProductStatus* st)
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
        if (chain_finish<Sum>(recs, blockIdx.x * kWaves + wid, ntiles, base / kTile, &row, &val) && lane == 0) write_y(y, u64(row), val, alpha, beta);
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        const u32 r = (blockIdx.x - chain_blocks) * kThreads + t;
        if (r >= rows) return;
        const u32 b = ro[r], e = ro[r + 1];
        if (b == e) write_y(y, u64(r), Sum::ident(), alpha, beta);
        else if (b / kTile == (e - 1u) / kTile) write_y(y, u64(r), sums[r], alpha, beta);  // (else: the chain above)
    } else {
        double total;
        u32 split;
        if (totals_finish<Sum>(recs, ntiles, s_w, s_split, &total, &split)) st->rows_split = split;
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int spmv_run(TileScratch* sc, hipStream_t s, double alpha, const speck_dcsr* A, const double* d_x, double beta, double* d_y,
             ProductStatus* h)
{
    const u32 rows = (u32)A->rows;
    TileWork<ProductStatus> w;
    int rc = carve_and_check(sc, s, A, 1, rows, &w);
    if (rc != SPECK_OK) return rc;
    if (w.max_tiles) {
        const SpmvArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), d_x, w.sums, A->nnz, rows, (u32)A->cols,
                            on_16_bytes(A->data) && on_16_bytes(A->col_ids) ? 1u : 0u, w.recs, w.tile_rows, w.st};
        SPECK_LAUNCH(spmv_tile_kernel<T>, dim3(w.max_tiles), dim3(kThreads), 0, s, g);
    }
    const u32 chain_blocks = (w.max_tiles + kWaves - 1) / kWaves, row_blocks = (rows + kThreads - 1) / kThreads;
    SPECK_LAUNCH(spmv_finish_kernel, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 chain_blocks, row_blocks, w.sums, w.recs, alpha, beta, d_y, w.st);
    // the ONE read-back of the call: the two verdicts, the counters
    rc = read_status(s, w.st, h);
    if (rc != SPECK_OK) return rc;
    return (h->invalid || h->bad_id) ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kGuardNames[3] = {"spmv status", "spmv tile records and rows", "spmv row sums"};

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
    ProductStatus h{};
    const int rc = run_tile_call(cfg, spmv_scratch, kGuardNames, 3, " by the matrix-vector product", [&](TileScratch* sc, hipStream_t s) {
        return spmv_run<T>(sc, s, alpha, A, d_x, beta, d_y, &h);
    });
    if (rc != SPECK_OK) return rc;
    if (info) fill_tile_info(info, h, A);
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
