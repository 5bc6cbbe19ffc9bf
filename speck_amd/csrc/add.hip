// add.hip -- speck_add_*: C = alpha A + beta B on the union of the two patterns, rows ascending, every value computed in
// double without a fused multiply-add and rounded once.  The reference has no counterpart.
//
//   add_mark_kernel    tiles of 256 or 1024 rows, the tile's offsets of A and of B in LDS and checked first (the offset
//                      check: row_tiles.hpp), then a thread per entry of A and per entry of B, four loads in flight: the
//                      entry against its predecessor in the row and against cols, and its lower bound in the other
//                      operand's row, between that row's checked bounds -- no offset or id is used as an address before it
//                      was checked.  Writes one "also in the other operand" byte and that lower bound per entry, and
//                      len A + len B - matches per row; the matches are counted in LDS and reach the status block with one
//                      atomic per workgroup.
//   between            entries per row -> the shared scan (scan.hpp) -> the row offsets of C and nnz(C), queued behind the
//                      marking pass (temporaries only): the host reads the verdict and nnz(C) in ONE read-back, and every
//                      kernel that writes C starts after it.
//   add_write_kernel   once per operand, 4096 entries per workgroup, four per thread as the compaction places them
//                      (compact.hpp).  An entry's place in its row of C is its index in its own row + its lower bound in the
//                      other operand's row - the matches in front of it in its row; with the row offsets of C written out
//                      every row offset cancels, and entry e of X lands at e + (its lower bound in Y, counted from Y's first
//                      entry) - (the matches in front of it in X): the shared scan over the match bytes (a word of four per
//                      item) + a block scan.  The lower bound is the one the marking pass stored (searching again was
//                      measured and lost).  A matching entry of A carries alpha a + beta b, a matching entry
//                      of B writes nothing: every place of C is written exactly once, no atomics on values.
// The host side is the side operations' own (side_call.hpp: scratch, status, the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "add.hpp"
#include "compact.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scan.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kTileLong = SPECK_ADD_TILE_ROWS_LONG, kTileShort = SPECK_ADD_TILE_ROWS_SHORT;
constexpr u32 kMarkUnroll = 4;
constexpr u32 kWriteTile = SPECK_ADD_TILE_ENTRIES;
static_assert(kWriteTile == kCompactTile, "the write pass places its entries from the scan the compaction uses");

struct AddStatus {
    u32 invalid;               // offsets of A / B
    u32 unsorted;              // a row of A / B not strictly ascending, or an id >= cols
    u32 base_a, base_b;        // row_offsets[0]
    u32 entries_a, entries_b;  // row_offsets[rows] - row_offsets[0]: the entries the rows hold (== nnz, or the call is refused)
    unsigned long long both, nnz_out;
};

struct AddMarkArgs {
    const u32 *a_ro, *a_col;
    u64 a_nnz;
    const u32 *b_ro, *b_col;
    u64 b_nnz;
    u32 rows, cols;
    u8 *match_a, *match_b;          // one byte per entry (entry e of the buffers at e - row_offsets[0])
    u32 *lb_a, *lb_b;               // ... and its lower bound in the other operand's row (an absolute offset)
    u32* row_cnt;                   // entries of C per row
    AddStatus* st;
};

// ------------------------------------------------------------------------------------------------ check + mark
// The entries of operand X in the tile's rows, a batch of kMarkUnroll per thread (every thread makes the same trips: the
// waves stay whole for count_entry_in_row).  The row of an entry: first_end_beyond over the tile's offsets.  Its column is
// looked up in Y's row between that row's checked bounds (lower_bound_in_row).
// kCount (X = A): the matches per row into s_cnt.  Returns "a row of X is not strictly ascending below cols".
template <u32 kTileRows, bool kCount>
__device__ __forceinline__ bool add_mark_operand(const u32* __restrict__ x_col, const u32* s_xro, const u32* __restrict__ y_col,
                                                 const u32* s_yro, u32 nr, u32 cols, u32 base_x, u8* __restrict__ match,
                                                 u32* __restrict__ lbs, u32* s_cnt)
{
    const u32 t = threadIdx.x;
    bool unsorted = false;
    const u64 lo = s_xro[0], hi = s_xro[nr];
    for (u64 b = lo; b < hi; b += u64(kTileRows) * kMarkUnroll) {
        u32 c[kMarkUnroll], p[kMarkUnroll];
#pragma unroll
        for (u32 k = 0; k < kMarkUnroll; ++k) {
            const u64 i = b + k * kTileRows + t;
            c[k] = i < hi ? x_col[i] : 0u;
            p[k] = i < hi && i > lo ? x_col[i - 1] : 0u;
        }
#pragma unroll
        for (u32 k = 0; k < kMarkUnroll; ++k) {
            const u64 i = b + k * kTileRows + t;
            const bool valid = i < hi;
            const u32 r = valid ? first_end_beyond(s_xro + 1, nr, i) : nr - 1u;  // the row of entry i (< nr: i < s_xro[nr])
            unsorted |= valid && (c[k] >= cols || (i > s_xro[r] && p[k] >= c[k]));
            // (offsets relative to y_col as they stand: absolute, checked by the caller)
            const u32 yend = valid ? s_yro[r + 1] : s_yro[r], ylo = lower_bound_in_row(y_col, s_yro[r], yend, c[k]);
            const bool m = ylo < yend && y_col[ylo] == c[k];
            if (valid) {
                const u32 e = (u32)i - base_x;
                match[e] = m ? 1 : 0;
                lbs[e] = ylo;
            }
            if (kCount) count_entry_in_row(s_cnt, r, m);
        }
    }
    return unsorted;
}

// kTileRows rows and kTileRows threads per workgroup: 1024 where rows are short, 256 where a row of A and of B together
// hold 32 entries or more on average.
template <u32 kTileRows>
__global__ __launch_bounds__(kTileRows) void add_mark_kernel(const AddMarkArgs g)
{
    SPECK_POISON();
    __shared__ u32 s_aro[kTileRows + 1];
    __shared__ u32 s_bro[kTileRows + 1];
    __shared__ u32 s_cnt[kTileRows];  // matches per row
    __shared__ u32 s_bad;
    __shared__ unsigned long long s_both;
    const u32 t = threadIdx.x;
    const u32 r0 = blockIdx.x * kTileRows;
    const u32 nr = min(kTileRows, g.rows - r0);
    const u32 base_a = g.a_ro[0], base_b = g.b_ro[0];
    if (t == 0) s_bad = 0, s_both = 0;
    s_cnt[t] = 0;
    if (t == 0 && blockIdx.x == 0) g.st->base_a = base_a, g.st->base_b = base_b;
    __syncthreads();
    tile_offsets_load<kTileRows>(g.a_ro, r0, nr, base_a, g.a_nnz, s_aro, &s_bad);
    tile_offsets_load<kTileRows>(g.b_ro, r0, nr, base_b, g.b_nnz, s_bro, &s_bad);
    __syncthreads();
    if (tile_offsets_descend(s_aro, nr) || tile_offsets_descend(s_bro, nr)) s_bad = 1;
    __syncthreads();
    if (s_bad) {  // (nothing of col_ids is addressed through such offsets)
        if (t == 0) g.st->invalid = 1;
        return;
    }
    if (t == 0 && r0 + nr == g.rows) g.st->entries_a = s_aro[nr] - base_a, g.st->entries_b = s_bro[nr] - base_b;
    bool unsorted = add_mark_operand<kTileRows, true>(g.a_col, s_aro, g.b_col, s_bro, nr, g.cols, base_a, g.match_a, g.lb_a, s_cnt);
    unsorted |= add_mark_operand<kTileRows, false>(g.b_col, s_bro, g.a_col, s_aro, nr, g.cols, base_b, g.match_b, g.lb_b, nullptr);
    if (unsorted) g.st->unsorted = 1;
    __syncthreads();
    u32 both = 0;
    if (t < nr) {
        both = s_cnt[t];
        g.row_cnt[r0 + t] = (s_aro[t + 1] - s_aro[t]) + (s_bro[t + 1] - s_bro[t]) - both;  // (both <= either length)
    }
    block_counter_to(&g.st->both, both, &s_both);
}

// ------------------------------------------------------------------------------------------------ values
// Each product rounded to double, the sum rounded to double, then once to T: alpha * a.astype(f64) + beta * b.astype(f64)
// in numpy.  The contraction is switched off where the operations are written: the flag travels with them when the
// functions are inlined.  (The multiply needs nothing of the kind: its products meet their sums through LDS atomics.)
template <typename T>
__device__ __forceinline__ T add_scaled(double cx, T x)
{
#pragma clang fp contract(off)
    return (T)(cx * (double)x);
}

template <typename T>
__device__ __forceinline__ T add_both(double cx, T x, double cy, T y)
{
#pragma clang fp contract(off)
    const double px = cx * (double)x;
    const double py = cy * (double)y;
    const double sum = px + py;
    return (T)sum;
}

// ------------------------------------------------------------------------------------------------ write
template <typename T>
struct AddWriteArgs {
    const u32* x_col;       // the operand whose entries this launch places, from its first entry (row_offsets[0]) on
    const T* x_val;
    const T* y_val;         // the other one, as its buffer stands (the lower bounds are absolute offsets)
    double cx, cy;          // the coefficients of X and of Y
    KeepWord words;         // the match bytes of X
    const u32* tile_sums;   // their scanned sums per tile
    const u32* lbs;         // the lower bound of every entry of X in its row of Y
    u32 base_y;             // Y.row_offsets[0]
    u32* c_col;
    T* c_val;
};

// 4096 entries of X per workgroup, four per thread, numbered by the scan that compact_entries_kernel (compact.hpp) numbers
// its own by.  Entry e of X (counted from the first row on) in row r lands at
//     cro[r] + (its index in its row) + (its lower bound in Y's row - yro[r]) - (the matches in front of it in its row),
// and with cro[r] = (xro[r] - xro[0]) + (yro[r] - yro[0]) - (the matches in the rows before r) every row offset cancels:
//     place = e + (lower bound - yro[0]) - (the matches in front of it in X)
// -- the entries of X before it, the entries of Y before it, less what both count.  No row is looked up here.
template <typename T, bool kFirst>
__global__ __launch_bounds__(1024) void add_write_kernel(const AddWriteArgs<T> g)
{
    SPECK_POISON();
    __shared__ u32 s_scan[1024 / 64 + 1];
    const u32 i = blockIdx.x * 1024u + threadIdx.x;
    const u64 e0 = u64(i) * 4;
    const u32 w = g.words.word(i);
    u32 total;
    u32 seen = g.tile_sums[blockIdx.x] + block_exclusive_scan<1024>((u32)__popc(w), s_scan, &total);
    u32 c[4], lb[4];
    T v[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const bool valid = e0 + k < g.words.n;
        c[k] = valid ? g.x_col[e0 + k] : 0u;
        v[k] = valid ? g.x_val[e0 + k] : T(0);
        lb[k] = valid ? g.lbs[e0 + k] : 0u;
    }
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const bool m = (w >> (8u * k)) & 1u;
        if (e0 + k < g.words.n) {
            const u32 to = (u32)e0 + k + (lb[k] - g.base_y) - seen;
            if (kFirst) {
                g.c_col[to] = c[k];
                g.c_val[to] = m ? add_both<T>(g.cx, v[k], g.cy, g.y_val[lb[k]]) : add_scaled<T>(g.cx, v[k]);
            } else if (!m) {
                g.c_col[to] = c[k];
                g.c_val[to] = add_scaled<T>(g.cx, v[k]);
            }
        }
        seen += m;
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int add_run(AddScratch* sc, hipStream_t s, double alpha, const speck_dcsr* A, double beta, const speck_dcsr* B, speck_dcsr* C,
            speck_add_info* info, COut* out)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz_a = A->nnz, nnz_b = B->nnz;
    if (rows == 0) return publish_empty_c(C, A->cols, sizeof(T), s, out);

    // status | entries of C per row | the row offsets of C | workgroup sums of the scan
    RowScratch<AddStatus> f;
    int rc = carve_row_scratch(&sc->fixed, rows, 0, &f);
    if (rc != SPECK_OK) return rc;
    AddStatus* st = f.st;
    // per operand: match bytes | matches per tile of the write pass | lower bounds
    const u64 tiles_a = (nnz_a + kWriteTile - 1) / kWriteTile, tiles_b = (nnz_b + kWriteTile - 1) / kWriteTile;
    const size_t match_a_bytes = up256(std::max<u64>(nnz_a, 1)), match_b_bytes = up256(std::max<u64>(nnz_b, 1));
    const size_t tile_a_bytes = up256(size_t(std::max<u64>(tiles_a, 1)) * 4), tile_b_bytes = up256(size_t(std::max<u64>(tiles_b, 1)) * 4);
    const size_t lb_a_bytes = up256(std::max<u64>(nnz_a, 1) * 4), lb_b_bytes = up256(std::max<u64>(nnz_b, 1) * 4);
    rc = sc->var.ensure(match_a_bytes + match_b_bytes + tile_a_bytes + tile_b_bytes + lb_a_bytes + lb_b_bytes);
    if (rc != SPECK_OK) return rc;
    unsigned char* vb = static_cast<unsigned char*>(sc->var.p);
    u8* match_a = vb;
    u8* match_b = match_a + match_a_bytes;
    u32* sums_a = reinterpret_cast<u32*>(match_b + match_b_bytes);
    u32* sums_b = reinterpret_cast<u32*>(reinterpret_cast<unsigned char*>(sums_a) + tile_a_bytes);
    u32* lb_a = reinterpret_cast<u32*>(reinterpret_cast<unsigned char*>(sums_b) + tile_b_bytes);
    u32* lb_b = reinterpret_cast<u32*>(reinterpret_cast<unsigned char*>(lb_a) + lb_a_bytes);

    // ---- the verdict on A and B, the marks and nnz(C): read before anything of C is written
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(AddStatus), s));
    const AddMarkArgs g{A->row_offsets, A->col_ids, nnz_a, B->row_offsets, B->col_ids, nnz_b, rows, (u32)A->cols,
                        match_a, match_b, lb_a, lb_b, f.row_cnt, st};
    if ((nnz_a + nnz_b) / rows >= SPECK_ADD_LONG_ROW_AVG)
        SPECK_LAUNCH((add_mark_kernel<kTileLong>), dim3((rows + kTileLong - 1) / kTileLong), dim3(kTileLong), 0, s, g);
    else
        SPECK_LAUNCH((add_mark_kernel<kTileShort>), dim3((rows + kTileShort - 1) / kTileShort), dim3(kTileShort), 0, s, g);
    // (on a refused input the counts of a tile may be missing: the scan adds up whatever the words hold and addresses
    //  nothing through them)
    launch_exclusive_scan(s, CountArray{f.row_cnt}, rows, f.block_sums, f.new_ro, &st->nnz_out);
    AddStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    // (the last offset of each operand spans its nnz, as for speck_reduce_*)
    if (h.invalid || h.entries_a != A->nnz || h.entries_b != B->nnz) return SPECK_ERR_INVALID;
    if (h.unsorted) return SPECK_ERR_UNSORTED;

    // ---- write
    const u64 nnz_out = h.nnz_out;
    rc = prepare_c(C, rows, nnz_out, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    const T *va = static_cast<const T*>(A->data), *vb_ = static_cast<const T*>(B->data);
    if (h.entries_a) {
        const KeepWord words{reinterpret_cast<const u32*>(match_a), h.entries_a};
        launch_exclusive_scan(s, words, (u32)((u64(h.entries_a) + 3) / 4), sums_a, nullptr, nullptr);
        const AddWriteArgs<T> w{A->col_ids + h.base_a, va + h.base_a, vb_, alpha, beta, words, sums_a, lb_a, h.base_b,
                                out->col, static_cast<T*>(out->val)};
        SPECK_LAUNCH((add_write_kernel<T, true>), dim3((u32)((u64(h.entries_a) + kWriteTile - 1) / kWriteTile)), dim3(1024), 0, s, w);
    }
    if (h.entries_b) {
        const KeepWord words{reinterpret_cast<const u32*>(match_b), h.entries_b};
        launch_exclusive_scan(s, words, (u32)((u64(h.entries_b) + 3) / 4), sums_b, nullptr, nullptr);
        const AddWriteArgs<T> w{B->col_ids + h.base_b, vb_ + h.base_b, va, beta, alpha, words, sums_b, lb_b, h.base_a,
                                out->col, static_cast<T*>(out->val)};
        SPECK_LAUNCH((add_write_kernel<T, false>), dim3((u32)((u64(h.entries_b) + kWriteTile - 1) / kWriteTile)), dim3(1024), 0, s, w);
    }
    rc = finish_rows(s, f.new_ro, rows, A->cols, nnz_out, C, out);
    if (rc != SPECK_OK) return rc;
    if (info) {
        info->both = h.both;
        info->only_a = h.entries_a - h.both;
        info->only_b = h.entries_b - h.both;
        info->nnz_out = nnz_out;
    }
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"add row counts", "add match bytes", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int add_impl(speck_config* cfg, double alpha, const speck_dcsr* A, double beta, const speck_dcsr* B, speck_dcsr* C, int flags,
             speck_add_info* info)
{
    if (!A || !B || !C) return SPECK_ERR_INVALID;
    if (flags != SPECK_ADD_UNION) return SPECK_ERR_INVALID;
    if (A->rows != B->rows || A->cols != B->cols) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    // (conservative: an overlap might have fitted -- but this is known without a device, and every count stays in 32 bits)
    if (A->nnz >= (1ull << 32) || B->nnz >= (1ull << 32) || A->nnz + B->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (!csr_args_ok(A, true) || !csr_args_ok(B, true)) return SPECK_ERR_INVALID;
    if (shares_buffer(C, A) || shares_buffer(C, B)) return SPECK_ERR_INVALID;
    if (info) *info = speck_add_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, add_scratch, C, info, kGuardNames, " by the addition", [&](AddScratch* sc, hipStream_t s, COut* out) {
        return add_run<T>(sc, s, alpha, A, beta, B, C, info, out);
    });
}

}  // namespace

extern "C" {

int speck_add_f64(speck_config* cfg, double alpha, const speck_dcsr* A, double beta, const speck_dcsr* B, speck_dcsr* C, int flags,
                  speck_add_info* info)
{
    return add_impl<double>(cfg, alpha, A, beta, B, C, flags, info);
}

int speck_add_f32(speck_config* cfg, double alpha, const speck_dcsr* A, double beta, const speck_dcsr* B, speck_dcsr* C, int flags,
                  speck_add_info* info)
{
    return add_impl<float>(cfg, alpha, A, beta, B, C, flags, info);
}

}  // extern "C"
