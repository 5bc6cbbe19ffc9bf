// side_call.hpp -- the host side of what the side operations (sort_rows.hip, masked.hip, select.hip, add.hip) share beside
// C's buffers (compact.hpp): how a call carves its fixed scratch, reads its status block, checks the canary zones (debug
// option guard_bytes), and the frame around its body.  (The calls that hand over no C but a vector -- reduce, spmv, spmm --
// have theirs in tile_call.hpp, which takes read_status from here.)
#pragma once
#include "compact.hpp"
#include "launch.hpp"

namespace speck {

// The `fixed` buffer of an operation whose result has rows of new lengths, sized from `rows` before the first kernel:
// status block | lists | counts per row | new row offsets | scan sums, regions of multiples of 256 bytes.
template <typename Status>
struct RowScratch {
    Status* st;
    u32* lists;       // list_words words (may be 0)
    u32* row_cnt;     // rows + 1
    u32* new_ro;      // rows + 1
    u32* block_sums;  // one per 1024 rows (scan.hpp)
};

template <typename Status>
int carve_row_scratch(DeviceBuffer* fixed, u32 rows, size_t list_words, RowScratch<Status>* out)
{
    static_assert(sizeof(Status) <= 256, "status block");
    const size_t list_bytes = up256(list_words * 4), row_bytes = up256((size_t(rows) + 1) * 4);
    const size_t sum_bytes = up256(size_t((rows + 1023) / 1024) * 4);
    const int rc = fixed->ensure(256 + list_bytes + 2 * row_bytes + sum_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* fb = static_cast<unsigned char*>(fixed->p);
    out->st = reinterpret_cast<Status*>(fb);
    out->lists = reinterpret_cast<u32*>(fb + 256);
    out->row_cnt = reinterpret_cast<u32*>(fb + 256 + list_bytes);
    out->new_ro = reinterpret_cast<u32*>(fb + 256 + list_bytes + row_bytes);
    out->block_sums = reinterpret_cast<u32*>(fb + 256 + list_bytes + 2 * row_bytes);
    return SPECK_OK;
}

// what the kernels queued on `s` so far left in the status block: the ONE place a call waits for its verdict
template <typename Status>
int read_status(hipStream_t s, const Status* st, Status* h)
{
    HIP_TRY(hipMemcpyAsync(h, st, sizeof *h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return take_launch_error() ? SPECK_ERR_HIP : SPECK_OK;
}

// names: of the two temporaries and of X's data, col_ids and row_offsets, as stderr shows them; whose: " by the row sort"
template <typename Scratch>
int check_side_guards(const Scratch* sc, hipStream_t s, const speck_dcsr* X, const char* const names[5], const char* whose, int rc)
{
    const void* whole[] = {sc->fixed.p, sc->var.p, X->data, X->col_ids, X->row_offsets};
    return guard_check_buffers(whole, names, 5, s, whose, rc);
}

// The frame of an entry point that makes a new C: run(scratch, stream, out) is the body.  Where it fails, what it allocated
// for C and never handed over is freed and `info` is zero again.
template <typename Scratch, typename Info, typename Run>
int run_side_call(speck_config* cfg, Scratch* (*scratch_of)(speck_config*), const speck_dcsr* C, Info* info,
                  const char* const guard_names[5], const char* whose, Run&& run)
{
    Scratch own;
    Scratch* sc = cfg ? scratch_of(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    COut out;
    int rc = run(sc, s, &out);
    if (rc != SPECK_OK) {
        (void)hipStreamSynchronize(s);
        out.discard();
        if (info) *info = Info{};
    }
    rc = check_side_guards(sc, s, C, guard_names, whose, rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    return rc;
}

}  // namespace speck
