// tile_call.hpp -- the host side of what the operations over ENTRY TILES with a vector for a result (reduce.hip, spmv.hip,
// spmm.hip) share, the sibling of side_call.hpp for calls that hand over no C: how a call carves its scratch and queues
// the check of the offsets (carve_and_check), the frame around its body (run_tile_call), and the counts every one of
// them reports (fill_tile_info).  The device side is tile_combine.hpp.
#pragma once
#include "side_call.hpp"
#include "tile_combine.hpp"
#include "tile_scratch.hpp"

namespace speck {

// what carve_and_check carved and queued the check for
template <typename Status>
struct TileWork {
    Status* st;                    // cleared; tile_check_kernel fills invalid, base and rows_empty
    tile_combine::TileRec* recs;   // `sets` records per tile: those of set c start at recs + c max_tiles
    u32* tile_rows;                // two words per tile: the rows of its first and of its last entry
    double* sums;                  // sum_doubles doubles (null where none were asked for)
    u32 max_tiles;                 // the tiles A touches at most: the grid of the tile kernel
};

// The first steps of a call on `s`: the three buffers of `sc` sized for A, `sets` records per tile and sum_doubles row
// sums; the status block cleared; tile_check_kernel queued.  Status: tile_check_kernel's contract.
template <typename Status>
int carve_and_check(TileScratch* sc, hipStream_t s, const speck_dcsr* A, u32 sets, size_t sum_doubles, TileWork<Status>* w)
{
    using namespace tile_combine;
    static_assert(sizeof(Status) <= 256, "status block");
    const u32 rows = (u32)A->rows;
    w->max_tiles = entry_tiles_at_most(A->nnz, kTile);
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    const size_t rec_bytes = up256(size_t(std::max(w->max_tiles, 1u)) * sets * sizeof(TileRec));
    rc = sc->var.ensure(rec_bytes + up256(size_t(std::max(w->max_tiles, 1u)) * 8));
    if (rc != SPECK_OK) return rc;
    if (sum_doubles) {
        rc = sc->sums.ensure(up256(sum_doubles * 8));
        if (rc != SPECK_OK) return rc;
    }
    w->st = static_cast<Status*>(sc->fixed.p);
    w->recs = static_cast<TileRec*>(sc->var.p);
    w->tile_rows = reinterpret_cast<u32*>(static_cast<unsigned char*>(sc->var.p) + rec_bytes);
    w->sums = sum_doubles ? static_cast<double*>(sc->sums.p) : nullptr;

    HIP_TRY(hipMemsetAsync(w->st, 0, sizeof(Status), s));
    SPECK_LAUNCH(tile_check_kernel<Status>, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 w->max_tiles, w->tile_rows, w->st);
    return SPECK_OK;
}

// The frame of an entry point whose result is a vector the caller owns: run(scratch, stream) is the body.  guard_names:
// of fixed, var and sums, as stderr shows them, the first n_guards of them checked; whose: " by the reduction".
template <typename Run>
int run_tile_call(speck_config* cfg, TileScratch* (*scratch_of)(speck_config*), const char* const* guard_names, int n_guards,
                  const char* whose, Run&& run)
{
    TileScratch own;
    TileScratch* sc = cfg ? scratch_of(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    int rc = run(sc, s);
    if (rc != SPECK_OK) (void)hipStreamSynchronize(s);
    const void* whole[] = {sc->fixed.p, sc->var.p, sc->sums.p};
    rc = guard_check_buffers(whole, guard_names, n_guards, s, whose, rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    return rc;
}

// the four counts of speck_reduce_info, speck_spmv_info and speck_spmm_info, from the status block read back
template <typename Info, typename Status>
void fill_tile_info(Info* info, const Status& h, const speck_dcsr* A)
{
    info->rows_empty = h.rows_empty;
    info->rows_split = h.rows_split;
    info->tiles = tile_combine::tiles_touched(h.base, A->nnz);
    info->entries = A->nnz;
}

}  // namespace speck
