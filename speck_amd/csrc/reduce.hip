// reduce.hip -- speck_reduce_*: per row and over all entries of a device CSR, the sum of v, |v| or v v, or the largest v,
// smallest v or largest |v|, in double.  Reads row_offsets and data, never col_ids.  The reference has no counterpart.
//
//   tile_check_kernel      (tile_combine.hpp) a thread per row: the offsets ascend, stay inside [row_offsets[0],
//                          row_offsets[0] + nnz] and the last one spans nnz; counts the rows without an entry.  Raises
//                          the verdict in the status block.
//                          A row that holds the first or the last entry of a tile says so in the tile's two words: the
//                          tile pass searches nothing (a search was four dependent loads in front of every tile).  The
//                          check of a row is entry_tiles.hpp's: the scaling walks the same tiles.
//   reduce_tile_kernel     queued behind it, looks at the verdict first (and does nothing where it is raised: no offset is
//                          used as an address before it was checked, and there is no read-back in between).  A workgroup
//                          per ENTRY TILE: the absolute entries [4096 t, 4096 (t + 1)) of `data`, clipped to the matrix.
//                          A thread holds 16 consecutive entries (16-byte loads); the rows that start in the tile are
//                          marked in a bitmap in LDS; then a segmented combine -- serially in the thread, across the
//                          lanes with DPP shifts, across the four waves through LDS.  A second walk over the tile's rows
//                          picks every row that ends in the tile from LDS and writes it; a row open at the tile's start or
//                          end leaves its partial in the tile's record, and the tile's own total goes there too.
//   reduce_finish_kernel   three kinds of workgroups in one launch: a wave per tile finishes the row that leaves the tile
//                          open (tail of its first tile, the whole tiles inside it, head of its last: a fixed tree over the
//                          tile numbers); a thread per row gives the rows without entries the identity; one workgroup
//                          combines the tile totals in a fixed tree into the status block and counts the split rows.
// Every combination tree depends on the absolute positions of the entries alone: a row-range view gives bit for bit the
// rows of the whole matrix, and a call gives the same bits every time.  No floating-point atomic.  A NaN is carried by
// the values themselves: the sums propagate it, and the extrema combine with "a > b or a is NaN ? a : b".
// The combine itself -- the walk in the thread, the DPP scan, the carry across the waves, the tile record and the chain
// finish -- lives in tile_combine.hpp, with a tile kernel's opening and the load of a thread's entries: spmv.hip and
// spmm.hip run the same tree over the terms a x[j].  The host side stands on tile_call.hpp, which the three share: the
// scratch, the check's launch, the frame of a call that hands over no C.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "launch.hpp"
#include "tile_call.hpp"

// every square and every sum is rounded on its own: all code paths add the same terms (add.hip does the same per function)
#pragma clang fp contract(off)

using namespace speck;

namespace {

using namespace speck::tile_combine;  // the segmented combine, its records and its check kernel: spmv.hip walks the same tree
static_assert(kTile == SPECK_REDUCE_TILE_ENTRIES && kPer == SPECK_REDUCE_THREAD_ENTRIES && 64 * kPer == SPECK_REDUCE_WAVE_ENTRIES,
              "the header's figures");

struct ReduceStatus {
    u32 invalid;  // the offsets
    u32 base;     // row_offsets[0]
    unsigned long long rows_empty, rows_split;
    double total;
};

// ------------------------------------------------------------------------------------------------ tiles
template <typename T>
struct ReduceArgs {
    const u32* ro;
    const T* data;
    u32 rows;
    u64 nnz;
    double* row_out;  // may be null
    TileRec* recs;
    const u32* tile_rows;
    ReduceStatus* st;
};

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void reduce_tile_kernel(const ReduceArgs<T> g)
{
    SPECK_POISON();
    using O = Op<OP>;
    __shared__ TileLds s_tile;
    if (g.st->invalid) return;  // (the verdict of tile_check_kernel: nothing below runs on offsets it refused)
    TileFrame f;
    if (!tile_frame(g.st->base, g.nnz, blockIdx.x, &f)) return;

    // the thread's 16 entries: their terms, the identity where the matrix does not reach (a whole tile asks nothing per entry)
    T a[kPer];
    load_entries<false>(f, f.whole, g.data, nullptr, a, nullptr);
    double v[kPer];
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) v[k] = O::term((double)a[k]);
    if (!f.whole) {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k)
            if (!entry_in(f, k)) v[k] = O::ident();
    }

    // (rows without entries: reduce_finish_kernel)
    double* const row_out = g.row_out;
    combine_tile<O>(s_tile, v, g.ro, g.tile_rows, g.recs + blockIdx.x, f.tile0, f.lo, f.hi, [row_out](u32 r, double val) {
        if (row_out) row_out[r] = val;
    });
}

// ------------------------------------------------------------------------------------------------ finish
template <int OP>
__global__ __launch_bounds__(kThreads) void reduce_finish_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 chain_blocks,
                                                                 u32 row_blocks, double* __restrict__ row_out,
                                                                 const TileRec* __restrict__ recs, ReduceStatus* st)
{
    SPECK_POISON();
    using O = Op<OP>;
    __shared__ double s_w[kWaves];
    __shared__ u32 s_split[kWaves];
    if (st->invalid) return;
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u64 base = st->base;
    const u32 ntiles = tiles_touched(base, nnz);
    if (blockIdx.x < chain_blocks) {
        u32 row;
        double val;
        if (chain_finish<O>(recs, blockIdx.x * kWaves + wid, ntiles, base / kTile, &row, &val) && lane == 0 && row_out) row_out[row] = val;
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        const u32 r = (blockIdx.x - chain_blocks) * kThreads + t;
        if (row_out && r < rows && ro[r] == ro[r + 1]) row_out[r] = O::ident();
    } else {
        double total;
        u32 split;
        if (totals_finish<O>(recs, ntiles, s_w, s_split, &total, &split)) {
            st->total = total;
            st->rows_split = split;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, int OP>
void reduce_launch(hipStream_t s, const speck_dcsr* A, double* d_row_out, const TileWork<ReduceStatus>& w)
{
    const u32 rows = (u32)A->rows;
    if (w.max_tiles) {
        const ReduceArgs<T> g{A->row_offsets, static_cast<const T*>(A->data), rows, A->nnz, d_row_out, w.recs, w.tile_rows, w.st};
        SPECK_LAUNCH((reduce_tile_kernel<T, OP>), dim3(w.max_tiles), dim3(kThreads), 0, s, g);
    }
    const u32 chain_blocks = (w.max_tiles + kWaves - 1) / kWaves, row_blocks = (rows + kThreads - 1) / kThreads;
    SPECK_LAUNCH(reduce_finish_kernel<OP>, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 chain_blocks, row_blocks, d_row_out, w.recs, w.st);
}

double identity_of(int op)
{
    return op == SPECK_REDUCE_MAX ? Op<SPECK_REDUCE_MAX>::ident() : op == SPECK_REDUCE_MIN ? Op<SPECK_REDUCE_MIN>::ident() : 0.0;
}

template <typename T>
int reduce_run(TileScratch* sc, hipStream_t s, const speck_dcsr* A, int op, double* d_row_out, ReduceStatus* h)
{
    TileWork<ReduceStatus> w;
    int rc = carve_and_check(sc, s, A, 1, 0, &w);
    if (rc != SPECK_OK) return rc;
    switch (op) {
    case SPECK_REDUCE_SUM: reduce_launch<T, SPECK_REDUCE_SUM>(s, A, d_row_out, w); break;
    case SPECK_REDUCE_ABS_SUM: reduce_launch<T, SPECK_REDUCE_ABS_SUM>(s, A, d_row_out, w); break;
    case SPECK_REDUCE_SQ_SUM: reduce_launch<T, SPECK_REDUCE_SQ_SUM>(s, A, d_row_out, w); break;
    case SPECK_REDUCE_MAX: reduce_launch<T, SPECK_REDUCE_MAX>(s, A, d_row_out, w); break;
    case SPECK_REDUCE_MIN: reduce_launch<T, SPECK_REDUCE_MIN>(s, A, d_row_out, w); break;
    default: reduce_launch<T, SPECK_REDUCE_ABS_MAX>(s, A, d_row_out, w); break;
    }
    // the ONE read-back of the call: the verdict, the counters, the total
    rc = read_status(s, w.st, h);
    if (rc != SPECK_OK) return rc;
    return h->invalid ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kGuardNames[2] = {"reduce status", "reduce tile records and rows"};

template <typename T>
int reduce_impl(speck_config* cfg, const speck_dcsr* A, int op, double* d_row_out, double* h_total, speck_reduce_info* info)
{
    if (!A || op < SPECK_REDUCE_SUM || op > SPECK_REDUCE_ABS_MAX) return SPECK_ERR_INVALID;
    if (!d_row_out && !h_total) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    // (col_ids is never read: it may be NULL)
    if ((A->rows && !A->row_offsets) || (A->nnz && !A->data) || (A->rows == 0 && A->nnz)) return SPECK_ERR_INVALID;
    if (d_row_out && is_one_of(d_row_out, A)) return SPECK_ERR_INVALID;
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0) {  // no row, no entry: the identity
        if (h_total) *h_total = identity_of(op);
        if (info) *info = speck_reduce_info{};
        return SPECK_OK;
    }
    ReduceStatus h{};
    const int rc = run_tile_call(cfg, reduce_scratch, kGuardNames, 2, " by the reduction",
                                 [&](TileScratch* sc, hipStream_t s) { return reduce_run<T>(sc, s, A, op, d_row_out, &h); });
    if (rc != SPECK_OK) {
        if (info) *info = speck_reduce_info{};
        return rc;
    }
    if (h_total) *h_total = h.total;
    if (info) fill_tile_info(info, h, A);
    return SPECK_OK;
}

}  // namespace

extern "C" {

int speck_reduce_f64(speck_config* cfg, const speck_dcsr* A, int op, double* d_row_out, double* h_total, speck_reduce_info* info)
{
    return reduce_impl<double>(cfg, A, op, d_row_out, h_total, info);
}

int speck_reduce_f32(speck_config* cfg, const speck_dcsr* A, int op, double* d_row_out, double* h_total, speck_reduce_info* info)
{
    return reduce_impl<float>(cfg, A, op, d_row_out, h_total, info);
}

}  // extern "C"
