// select.hip -- speck_select_*: C = the entries of A that every selected predicate keeps (BAND: a diagonal band,
// ABS: a magnitude, PATTERN: membership in the pattern of another matrix; each may be negated), in input order, copied
// bit for bit.  The reference has no counterpart.
//
//   select_mark_kernel   one streaming pass over the rows, tiles of 256 or 1024 rows with the tile's offsets in LDS and a
//                        thread per entry, four loads in flight: the input check of A and of the pattern (the offset
//                        check and the pattern's rows: row_tiles.hpp; ids of A < cols -- no offset or id is used as an
//                        address before it was checked) and the predicates.  Writes one keep byte per entry and the kept
//                        entries per row; `kept` and `rows_unchanged` are counted in LDS and reach the status block with
//                        one atomic per workgroup and counter.  The predicates are uniform branches on the flags: a call
//                        that does not select ABS never loads a value, one that does not select PATTERN never touches a
//                        pattern.
//   finish               kept per row -> the shared scan (scan.hpp) -> the new row offsets and the total; finish_subset
//                        (compact.hpp): the same scan over the keep bytes -> one streaming compaction.
// The scan over the rows is queued behind the marking pass -- it writes temporaries only --, so the host reads the verdict
// and nnz(C) in ONE read-back; every kernel that writes C starts after it.
// The host side is the side operations' own (side_call.hpp: scratch, status, the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "compact.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "select.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kTileLong = SPECK_SELECT_TILE_ROWS_LONG, kTileShort = SPECK_SELECT_TILE_ROWS_SHORT;
constexpr u32 kMarkUnroll = 4;
constexpr u32 kKnownFlags = SPECK_SELECT_BAND | SPECK_SELECT_ABS | SPECK_SELECT_PATTERN | SPECK_SELECT_NOT_BAND |
                            SPECK_SELECT_NOT_ABS | SPECK_SELECT_NOT_PATTERN;

struct SelectStatus {
    u32 invalid;    // offsets of A / the pattern, an id of A
    u32 unsorted;   // a pattern row
    u32 base_a;     // A.row_offsets[0]
    u32 unchanged;  // rows that kept every entry
    u32 entries;    // A.row_offsets[rows] - A.row_offsets[0]: the entries the rows hold (== nnz, or the call is refused)
    unsigned long long kept, nnz_out;
};

template <typename T>
struct SelectArgs {
    const u32 *a_ro, *a_col;
    const T* a_val;
    u64 a_nnz;
    const u32 *p_ro, *p_col;  // the pattern (PATTERN only)
    u64 p_nnz;
    u32 rows, cols, flags;
    long long band_lo, band_hi;
    u64 row_base;
    double threshold;
    u8* keep;        // one byte per entry of A (entry e of A's buffers at e - A.row_offsets[0])
    u32* row_cnt;    // kept entries per row
    SelectStatus* st;
};

// ------------------------------------------------------------------------------------------------ check + mark
// kTileRows rows and kTileRows threads per workgroup: 1024 where rows are short, 256 where a row holds 32 entries or more
// on average (a tile should hold enough entries to pay for its barriers, and there should be enough tiles for the
// machine).  The row of an entry: first_end_beyond over the tile's offsets.  A PATTERN entry looks its column up in the
// pattern's row between that row's checked bounds (lower_bound_in_row): A's row needs no order for it.
template <typename T, u32 kTileRows>
__global__ __launch_bounds__(kTileRows) void select_mark_kernel(const SelectArgs<T> g)
{
    SPECK_POISON();
    __shared__ u32 s_aro[kTileRows + 1];
    __shared__ u32 s_pro[kTileRows + 1];
    __shared__ u32 s_cnt[kTileRows];  // kept entries per row
    __shared__ u32 s_bad, s_unchanged;
    __shared__ unsigned long long s_kept;
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kTileRows;
    const u32 nr = min(kTileRows, g.rows - r0);
    const bool band = g.flags & SPECK_SELECT_BAND, mag = g.flags & SPECK_SELECT_ABS, pat = g.flags & SPECK_SELECT_PATTERN;
    const bool not_band = g.flags & SPECK_SELECT_NOT_BAND, not_mag = g.flags & SPECK_SELECT_NOT_ABS,
               not_pat = g.flags & SPECK_SELECT_NOT_PATTERN;
    const u32 base_a = g.a_ro[0], base_p = pat ? g.p_ro[0] : 0u;
    if (t == 0) s_bad = 0, s_unchanged = 0, s_kept = 0;
    s_cnt[t] = 0;
    if (t == 0 && blockIdx.x == 0) g.st->base_a = base_a;
    __syncthreads();
    tile_offsets_load<kTileRows>(g.a_ro, r0, nr, base_a, g.a_nnz, s_aro, &s_bad);
    if (pat) tile_offsets_load<kTileRows>(g.p_ro, r0, nr, base_p, g.p_nnz, s_pro, &s_bad);
    __syncthreads();
    if (tile_offsets_descend(s_aro, nr) || (pat && tile_offsets_descend(s_pro, nr))) s_bad = 1;
    __syncthreads();
    if (s_bad) {  // (nothing of col_ids is addressed through such offsets)
        if (t == 0) g.st->invalid = 1;
        return;
    }
    if (t == 0 && r0 + nr == g.rows) g.st->entries = s_aro[nr] - base_a;
    if (pat && !rows_ascending_below<kTileRows>(g.p_col, s_pro, nr, g.cols)) g.st->unsorted = 1;
    // the tile's entries of A, a batch of kMarkUnroll per thread (every thread makes the same trips: the waves stay whole
    // for count_entry_in_row)
    bool bad_a = false;
    const u64 lo = s_aro[0], hi = s_aro[nr];
    for (u64 b = lo; b < hi; b += u64(kTileRows) * kMarkUnroll) {
        u32 c[kMarkUnroll];
        T v[kMarkUnroll];
#pragma unroll
        for (u32 k = 0; k < kMarkUnroll; ++k) {
            const u64 i = b + k * kTileRows + t;
            c[k] = i < hi ? g.a_col[i] : 0u;
            v[k] = T(0);
            if (mag && i < hi) v[k] = g.a_val[i];
        }
#pragma unroll
        for (u32 k = 0; k < kMarkUnroll; ++k) {
            const u64 i = b + k * kTileRows + t;
            const bool valid = i < hi;
            const u32 r = valid ? first_end_beyond(s_aro + 1, nr, i) : nr - 1u;  // the row of entry i (< nr: i < s_aro[nr])
            bool keep = valid;
            bad_a |= valid && c[k] >= g.cols;
            if (band) {
                // (wraps instead of overflowing: row_base <= 2^62, the columns and rows are below 2^27)
                const long long d = (long long)(u64(c[k]) - (g.row_base + r0 + r));
                keep &= (d >= g.band_lo && d <= g.band_hi) != not_band;
            }
            if (mag) keep &= !(fabs((double)v[k]) <= g.threshold) != not_mag;
            if (pat && keep) {
                // (offsets relative to p_col as they stand: absolute, checked above)
                const u32 pend = s_pro[r + 1], at = lower_bound_in_row(g.p_col, s_pro[r], pend, c[k]);
                const bool in = at < pend && g.p_col[at] == c[k];
                keep = in != not_pat;
            }
            if (valid) g.keep[i - base_a] = keep ? 1 : 0;
            count_entry_in_row(s_cnt, r, keep);
        }
    }
    if (bad_a) g.st->invalid = 1;
    __syncthreads();
    u32 cnt = 0;
    bool same = false;
    if (t < nr) {
        cnt = s_cnt[t];
        g.row_cnt[r0 + t] = cnt;
        same = cnt == s_aro[t + 1] - s_aro[t];
    }
    const u64 m = __ballot(same);  // (a flag per row: counted from the ballot, not summed)
    if (lane_id() == 0 && m) atomicAdd(&s_unchanged, (u32)__popcll(m));
    wave_counter_to_lds(&s_kept, cnt);
    __syncthreads();
    lds_counter_to_status(&g.st->kept, &s_kept, 0u);
    lds_counter_to_status(&g.st->unchanged, &s_unchanged, 64u);  // (another wave's thread: the two atomics leave side by side)
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int select_run(SelectScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_select_params* p, speck_dcsr* C,
               speck_select_info* info, COut* out)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz = A->nnz;
    const bool pat = p->flags & SPECK_SELECT_PATTERN;
    if (rows == 0) return publish_empty_c(C, A->cols, sizeof(T), s, out);

    // status | kept per row | new row offsets | workgroup sums of the scan
    RowScratch<SelectStatus> f;
    int rc = carve_row_scratch(&sc->fixed, rows, 0, &f);
    if (rc != SPECK_OK) return rc;
    SelectStatus* st = f.st;
    // keep bytes | kept entries per tile of the compaction
    const size_t keep_bytes = up256(std::max<u64>(nnz, 1));
    const size_t tile_bytes = up256(size_t(std::max<u64>((nnz + kCompactTile - 1) / kCompactTile, 1)) * 4);
    rc = sc->var.ensure(keep_bytes + tile_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* vb = static_cast<unsigned char*>(sc->var.p);
    u8* keep = vb;
    u32* tile_sums = reinterpret_cast<u32*>(vb + keep_bytes);

    // ---- the verdict on A and the pattern, the marks and nnz(C): read before anything of C is written
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SelectStatus), s));
    const speck_dcsr* P = pat ? p->pattern : nullptr;
    const SelectArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), nnz,
                          P ? P->row_offsets : nullptr, P ? P->col_ids : nullptr, P ? P->nnz : 0, rows, (u32)A->cols,
                          p->flags, (long long)p->band_lo, (long long)p->band_hi, p->row_base, p->abs_threshold, keep,
                          f.row_cnt, st};
    if ((nnz + (P ? P->nnz : 0)) / rows >= SPECK_SELECT_LONG_ROW_AVG)
        SPECK_LAUNCH((select_mark_kernel<T, kTileLong>), dim3((rows + kTileLong - 1) / kTileLong), dim3(kTileLong), 0, s, g);
    else
        SPECK_LAUNCH((select_mark_kernel<T, kTileShort>), dim3((rows + kTileShort - 1) / kTileShort), dim3(kTileShort), 0, s, g);
    // (on a refused input the counts of a tile may be missing: the scan adds up whatever the words hold and addresses
    //  nothing through them)
    launch_exclusive_scan(s, CountArray{f.row_cnt}, rows, f.block_sums, f.new_ro, &st->nnz_out);
    SelectStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid || h.entries != A->nnz) return SPECK_ERR_INVALID;  // (the last offset spans nnz, as for speck_reduce_*)
    if (h.unsorted) return SPECK_ERR_UNSORTED;

    // ---- finish
    const u64 nnz_out = h.nnz_out;
    rc = prepare_c(C, rows, nnz_out, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    const KeepWord words{reinterpret_cast<const u32*>(keep), h.entries};
    rc = finish_subset<T, T>(s, words, tile_sums, A->col_ids + h.base_a, static_cast<const T*>(A->data) + h.base_a, f.new_ro, rows,
                             A->cols, nnz_out, C, out);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->kept = h.kept;
        info->dropped = h.entries - h.kept;
        info->rows_unchanged = h.unchanged;
        info->nnz_out = nnz_out;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"select row counts", "select keep bytes", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int select_impl(speck_config* cfg, const speck_dcsr* A, const speck_select_params* p, speck_dcsr* C, speck_select_info* info)
{
    if (!A || !p || !C) return SPECK_ERR_INVALID;
    const u32 f = p->flags;
    if (f & ~kKnownFlags) return SPECK_ERR_INVALID;
    if ((f >> 4) & ~f & 7u) return SPECK_ERR_INVALID;  // NOT_x without x
    if ((f & SPECK_SELECT_BAND) && (p->band_lo > p->band_hi || p->row_base > (1ull << 62))) return SPECK_ERR_INVALID;
    if ((f & SPECK_SELECT_ABS) && !(p->abs_threshold >= 0.0)) return SPECK_ERR_INVALID;  // (a NaN fails the compare too)
    const speck_dcsr* P = (f & SPECK_SELECT_PATTERN) ? p->pattern : nullptr;
    if ((f & SPECK_SELECT_PATTERN) && (!P || P->rows != A->rows || P->cols != A->cols)) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32) || (P && P->nnz >= (1ull << 32))) return SPECK_ERR_INVALID;
    if (!csr_args_ok(A, true) || (P && !csr_args_ok(P, false))) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A) || (P && shares_buffer(C, P))) return SPECK_ERR_INVALID;
    if (info) *info = speck_select_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, select_scratch, C, info, kGuardNames, " by the select",
                         [&](SelectScratch* sc, hipStream_t s, COut* out) { return select_run<T>(sc, s, A, p, C, info, out); });
}

}  // namespace

extern "C" {

int speck_select_f64(speck_config* cfg, const speck_dcsr* A, const speck_select_params* p, speck_dcsr* C, speck_select_info* info)
{
    return select_impl<double>(cfg, A, p, C, info);
}

int speck_select_f32(speck_config* cfg, const speck_dcsr* A, const speck_select_params* p, speck_dcsr* C, speck_select_info* info)
{
    return select_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
