// coo.hip -- speck_from_coo_*: device COO triplets (row, column, value; 4- or 8-byte ids, in any order) grouped by row
// into a device CSR, stable, every id checked before it is followed; speck_to_coo: the rows of a device CSR expanded
// into one row index per entry.  The reference converts on the host only (convert(CSR&, const COO&), source/CSR.cpp:173-212).
//
//   coo_check_kernel       one pass over the ids in tiles of 2048 entries, a thread holds 8 consecutive ones (16-byte
//                          loads: two 8-byte or four 4-byte ids each): every row id against rows, every column id against
//                          cols -- an 8-byte id is compared as an unsigned 64-bit number, so a negative one or one with a
//                          set upper word is above every limit --, the row ids non-descending (inside the thread, and
//                          against the id in front of the thread's first, whichever lane, wave or tile holds it), and the
//                          u32 row keys of the sort written, clamped to 0 where the id was refused.  Raises the verdict and
//                          the unsorted flag in the status block: the FIRST read-back.
//   sorted input           coo_copy_kernel: columns and values straight over (narrowed, ones where there are no values).
//   general input          coo_positions_kernel, the tree's radix sort of (row key, position) on the call's stream
//                          (radix_pairs.hpp; ceil(log2(rows) / 8) passes), coo_gather_kernel through the positions.
//   coo_offsets_kernel     a thread per row: the lower bound of the row in the sorted keys = its offset.
//   offset_stats_kernel    (scan.hpp) the rows without an entry and the longest row: the SECOND read-back, behind which C is
//                          published.
//   to_coo_check_kernel    a thread per row: the family's offset check (entry_tiles.hpp); where columns were asked for,
//                          one streaming pass over the ids of the entries [row_offsets[0], row_offsets[0] + nnz) against
//                          cols; the first thread compares the outputs' spans with those entries, whose place only the
//                          device knows.
//   to_coo_expand_kernel   queued behind it, does nothing where the verdict is raised.  A wave takes 64 rows at a time, a
//                          lane each: a row of up to 16 entries is written by its lane, a longer one takes the whole wave,
//                          lanes striding its entries.  The columns are widened in a streaming pass of their own.
// No atomic decides the order of anything: the order is the sort's (ranks from ballots and scans); the counters are integer.
// No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "compact.hpp"
#include "coo.hpp"
#include "entry_tiles.hpp"
#include "launch.hpp"
#include "radix_pairs.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kCooThreads = 256, kCooPer = 8, kCooTile = kCooThreads * kCooPer;
static_assert(kCooTile == SPECK_COO_TILE_ENTRIES, "the header's figure");
constexpr u32 kCooGrid = 2048;      // workgroups of the grid-stride kernels
constexpr u32 kCooShortRow = 16;    // to_coo: a row of up to this many entries is written by its lane

struct CooStatus {
    u32 invalid;   // from_coo: an id out of range; to_coo: the offsets, an id, an output inside A's entries
    u32 unsorted;  // from_coo: a row id below the one in front of it
    u32 max_row;   // from_coo: the longest row
    u32 base;      // to_coo: row_offsets[0]
    unsigned long long rows_empty;
};

// ------------------------------------------------------------------------------------------------ from_coo: check
// the thread's kCooPer ids from position i0 on, as unsigned 64-bit numbers; 0 behind the end
template <typename I, bool kVec>
__device__ __forceinline__ void load_ids(const I* __restrict__ p, u64 i0, u64 n, u64 (&v)[kCooPer])
{
    if (kVec && i0 + kCooPer <= n) {
        if constexpr (sizeof(I) == 8) {
            const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + i0);
#pragma unroll
            for (u32 k = 0; k < kCooPer / 2; ++k) {
                const ulonglong2 w = q[k];
                v[2 * k] = w.x, v[2 * k + 1] = w.y;
            }
        } else {
            const uint4* q = reinterpret_cast<const uint4*>(p + i0);
#pragma unroll
            for (u32 k = 0; k < kCooPer / 4; ++k) {
                const uint4 w = q[k];
                v[4 * k] = w.x, v[4 * k + 1] = w.y, v[4 * k + 2] = w.z, v[4 * k + 3] = w.w;
            }
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < kCooPer; ++k) v[k] = i0 + k < n ? (u64)p[i0 + k] : 0ull;
    }
}

// I: u32 or u64 (an int64_t id read as unsigned).  kVec: both id arrays start on 16 bytes.
template <typename I, bool kVec>
__global__ __launch_bounds__(kCooThreads) void coo_check_kernel(const I* __restrict__ row, const I* __restrict__ col, u64 nnz,
                                                                u32 rows, u32 cols, u32* __restrict__ keys, CooStatus* st)
{
    SPECK_POISON();
    const u64 i0 = (u64(blockIdx.x) * kCooThreads + threadIdx.x) * kCooPer;
    if (i0 >= nnz) return;
    u64 r[kCooPer], c[kCooPer];
    load_ids<I, kVec>(row, i0, nnz, r);
    load_ids<I, kVec>(col, i0, nnz, c);
    // the id in front of the thread's first one (only ever compared)
    u64 prev = i0 ? (u64)row[i0 - 1] : 0ull;
    bool bad = false, descends = false;
    u32 key[kCooPer];
#pragma unroll
    for (u32 k = 0; k < kCooPer; ++k) {
        const bool valid = i0 + k < nnz;
        bad |= valid && (r[k] >= rows || c[k] >= cols);
        descends |= valid && r[k] < prev;
        if (valid) prev = r[k];
        key[k] = r[k] < rows ? (u32)r[k] : 0u;  // (clamped: nothing sorts or counts by an id that was refused)
    }
    if (i0 + kCooPer <= nnz) {
        uint4* q = reinterpret_cast<uint4*>(keys + i0);
        q[0] = make_uint4(key[0], key[1], key[2], key[3]);
        q[1] = make_uint4(key[4], key[5], key[6], key[7]);
    } else {
#pragma unroll
        for (u32 k = 0; k < kCooPer; ++k)
            if (i0 + k < nnz) keys[i0 + k] = key[k];
    }
    if (bad) st->invalid = 1;
    if (descends) st->unsorted = 1;
}

// ------------------------------------------------------------------------------------------------ from_coo: the rest
__global__ void coo_positions_kernel(u32* __restrict__ pos, u32 n)
{
    SPECK_POISON();
    for (u64 i = u64(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += u64(gridDim.x) * blockDim.x) pos[i] = (u32)i;
}

// behind a clean verdict: every id fits 32 bits.  val == nullptr: ones.
template <typename I, typename T>
__global__ void coo_copy_kernel(const I* __restrict__ col, const T* __restrict__ val, u32 nnz, u32* __restrict__ c_col,
                                T* __restrict__ c_val)
{
    SPECK_POISON();
    for (u64 i = u64(blockIdx.x) * blockDim.x + threadIdx.x; i < nnz; i += u64(gridDim.x) * blockDim.x) {
        c_col[i] = (u32)col[i];
        c_val[i] = val ? val[i] : T(1);
    }
}

// ... pos: the sorted positions, each below nnz (the library's own)
template <typename I, typename T>
__global__ void coo_gather_kernel(const u32* __restrict__ pos, const I* __restrict__ col, const T* __restrict__ val, u32 nnz,
                                  u32* __restrict__ c_col, T* __restrict__ c_val)
{
    SPECK_POISON();
    for (u64 i = u64(blockIdx.x) * blockDim.x + threadIdx.x; i < nnz; i += u64(gridDim.x) * blockDim.x) {
        const u32 src = pos[i];
        c_col[i] = (u32)col[src];
        c_val[i] = val ? val[src] : T(1);
    }
}

// ro[r] = lower bound of r in the non-descending keys, r = 0 .. rows
__global__ void coo_offsets_kernel(const u32* __restrict__ keys, u32 nnz, u32 rows, u32* __restrict__ ro)
{
    SPECK_POISON();
    for (u64 r = u64(blockIdx.x) * blockDim.x + threadIdx.x; r <= rows; r += u64(gridDim.x) * blockDim.x) {
        u32 lo = 0, hi = nnz;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < (u32)r) lo = mid + 1; else hi = mid;
        }
        ro[r] = lo;
    }
}

template <typename I>
void launch_check(hipStream_t s, const speck_dcoo* coo, u32* keys, CooStatus* st)
{
    const I* row = static_cast<const I*>(coo->row_ids);
    const I* col = static_cast<const I*>(coo->col_ids);
    const dim3 grid((u32)((coo->nnz + kCooTile - 1) / kCooTile));
    if (on_16_bytes(row) && on_16_bytes(col))
        SPECK_LAUNCH((coo_check_kernel<I, true>), grid, dim3(kCooThreads), 0, s, row, col, coo->nnz, (u32)coo->rows, (u32)coo->cols, keys, st);
    else
        SPECK_LAUNCH((coo_check_kernel<I, false>), grid, dim3(kCooThreads), 0, s, row, col, coo->nnz, (u32)coo->rows, (u32)coo->cols, keys, st);
}

template <typename I, typename T>
void launch_fill(hipStream_t s, const speck_dcoo* coo, const u32* pos, COut* out)
{
    const I* col = static_cast<const I*>(coo->col_ids);
    const T* val = static_cast<const T*>(coo->data);
    const u32 nnz = (u32)coo->nnz;
    const dim3 grid(grid_of((u64(nnz) + 255) / 256, kCooGrid));
    if (pos) SPECK_LAUNCH((coo_gather_kernel<I, T>), grid, dim3(256), 0, s, pos, col, val, nnz, out->col, static_cast<T*>(out->val));
    else SPECK_LAUNCH((coo_copy_kernel<I, T>), grid, dim3(256), 0, s, col, val, nnz, out->col, static_cast<T*>(out->val));
}

// the radix passes rows of this many need: ceil(log2(rows) / 8) of 8 bits
unsigned key_bits(u64 rows)
{
    unsigned bits = 0;
    while ((1ull << bits) < rows) ++bits;
    return bits;
}

template <typename T>
int from_coo_run(CooScratch* sc, hipStream_t s, const speck_dcoo* coo, speck_dcsr* C, speck_from_coo_info* info, COut* out)
{
    const u32 rows = (u32)coo->rows, nnz = (u32)coo->nnz;
    const bool wide = coo->index_bytes == 8;
    // status | keys a | keys b | positions a | positions b | histogram: every size is known before the first kernel
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    const size_t n4 = up256(size_t(std::max(nnz, 1u)) * 4);
    rc = sc->var.ensure(4 * n4 + kRadixHistWords * 4);
    if (rc != SPECK_OK) return rc;
    CooStatus* st = static_cast<CooStatus*>(sc->fixed.p);
    unsigned char* vb = static_cast<unsigned char*>(sc->var.p);
    u32* keys_a = reinterpret_cast<u32*>(vb);
    u32* keys_b = reinterpret_cast<u32*>(vb + n4);
    u32* pos_a = reinterpret_cast<u32*>(vb + 2 * n4);
    u32* pos_b = reinterpret_cast<u32*>(vb + 3 * n4);
    u32* hist = reinterpret_cast<u32*>(vb + 4 * n4);

    // ---- the verdict on every id and the order of the row ids: read before anything of C is allocated or written
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(CooStatus), s));
    CooStatus h{};
    if (nnz) {
        if (wide) launch_check<u64>(s, coo, keys_a, st);
        else launch_check<u32>(s, coo, keys_a, st);
        rc = read_status(s, st, &h);
        if (rc != SPECK_OK) return rc;
        if (h.invalid) return SPECK_ERR_INVALID;
    }
    const bool sorted = !h.unsorted;
    const unsigned bits = sorted ? 0u : key_bits(rows);

    rc = prepare_c(C, rows, nnz, sizeof(T), out);
    if (rc != SPECK_OK) return rc;
    if (nnz) {
        const u32* keys = keys_a;
        const u32* pos = nullptr;
        if (!sorted) {
            SPECK_LAUNCH(coo_positions_kernel, dim3(grid_of((u64(nnz) + 255) / 256, kCooGrid)), dim3(256), 0, s, pos_a, nnz);
            const int res = radix_sort_pairs(keys_a, pos_a, keys_b, pos_b, nnz, bits, hist, s);
            note_launch_status(hipGetLastError(), "radix_sort_pairs");
            keys = res ? keys_b : keys_a;
            pos = res ? pos_b : pos_a;
        }
        if (wide) launch_fill<u64, T>(s, coo, pos, out);
        else launch_fill<u32, T>(s, coo, pos, out);
        SPECK_LAUNCH(coo_offsets_kernel, dim3(grid_of((u64(rows) + 256) / 256, 8192)), dim3(256), 0, s, keys, nnz, rows, out->ro);
    } else {
        HIP_TRY(hipMemsetAsync(out->ro, 0, (size_t(rows) + 1) * 4, s));
    }
    if (rows) SPECK_LAUNCH(offset_stats_kernel, dim3(grid_of((u64(rows) + 255) / 256, kCooGrid)), dim3(256), 0, s, out->ro, rows, &st->max_row, &st->rows_empty);
    // ---- the counters: the second read-back, behind everything that fills C
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    publish_c(C, rows, coo->cols, nnz, out);
    if (info) {
        info->entries = nnz;
        info->rows_empty = h.rows_empty;
        info->max_row_entries = h.max_row;
        info->sorted_input = sorted ? 1 : 0;
        info->sort_passes = (bits + 7) / 8;
    }
    return SPECK_OK;
}

const char* const kFromGuardNames[5] = {"from_coo status", "from_coo keys and positions", "C.data", "C.col_ids", "C.row_offsets"};

template <typename T>
int from_coo_impl(speck_config* cfg, const speck_dcoo* coo, speck_dcsr* C, speck_from_coo_info* info)
{
    if (!coo || !C) return SPECK_ERR_INVALID;
    if (coo->index_bytes != 4 && coo->index_bytes != 8) return SPECK_ERR_INVALID;
    if (coo->rows > (1ull << 27) || coo->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (coo->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (coo->nnz && (!coo->row_ids || !coo->col_ids || coo->rows == 0 || coo->cols == 0)) return SPECK_ERR_INVALID;
    // C's buffers, as far as C declares them, against the three input arrays
    const void* in[3] = {coo->row_ids, coo->col_ids, coo->data};
    const u64 in_len[3] = {coo->nnz * coo->index_bytes, coo->nnz * coo->index_bytes, coo->nnz * sizeof(T)};
    const void* mine[3] = {C->data, C->col_ids, C->row_offsets};
    const u64 mine_len[3] = {C->nnz * sizeof(T), C->nnz * 4, (C->rows + 1) * 4};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            if (spans_overlap(mine[a], mine_len[a], in[b], in_len[b])) return SPECK_ERR_INVALID;
    if (info) *info = speck_from_coo_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, coo_scratch, C, info, kFromGuardNames, " by the COO conversion",
                         [&](CooScratch* sc, hipStream_t s, COut* out) { return from_coo_run<T>(sc, s, coo, C, info, out); });
}

// ------------------------------------------------------------------------------------------------ to_coo
struct ToCooArgs {
    const u32 *ro, *col;  // col: null where no columns were asked for
    u32 rows, cols;
    u64 nnz, row_base;
    const void *a_col, *a_data;  // A->col_ids and A->data: compared with the outputs' spans only
    void *row_out, *col_out;
    u32 index_bytes;
    CooStatus* st;
};

// the walk of the expansion: a wave takes 64 rows at a time, lane l row r0 + l with the entries [a, b); f(j, l) for
// every entry j of the lane's row: by the lane itself where the row is short, by all lanes of the wave where it is long
template <typename F>
__device__ __forceinline__ void walk_row_entries(u32 a, u32 b, F&& f)
{
    const u32 lane = lane_id();
    const u32 len = b - a;
    if (len <= kCooShortRow)
        for (u64 j = a; j < b; ++j) f(j, lane);
    u64 m = __ballot(len > kCooShortRow);
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const u32 sa = __shfl(a, src), sb = __shfl(b, src);
        for (u64 j = u64(sa) + lane; j < sb; j += 64) f(j, (u32)src);  // (64 bits: a view's offsets may end at 2^32 - 1)
    }
}

__global__ __launch_bounds__(256) void to_coo_check_kernel(const ToCooArgs g)
{
    SPECK_POISON();
    const u32 base = g.ro[0];
    bool bad = false;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g.st->base = base;
        // the outputs against A's entries: [base, base + nnz) of col_ids, and of data whichever of the two value types it holds
        const uintptr_t outs[2] = {reinterpret_cast<uintptr_t>(g.row_out), reinterpret_cast<uintptr_t>(g.col_out)};
        const u64 out_len = g.nnz * g.index_bytes;
        const uintptr_t c0 = reinterpret_cast<uintptr_t>(g.a_col) + u64(base) * 4;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(g.a_data) + u64(base) * 4, d1 = reinterpret_cast<uintptr_t>(g.a_data) + (u64(base) + g.nnz) * 8;
        for (int k = 0; k < 2; ++k) {
            if (!outs[k]) continue;
            if (g.a_col && outs[k] < c0 + g.nnz * 4 && c0 < outs[k] + out_len) bad = true;
            if (g.a_data && outs[k] < d1 && d0 < outs[k] + out_len) bad = true;
        }
    }
    for (u64 r = u64(blockIdx.x) * blockDim.x + threadIdx.x; r < g.rows; r += u64(gridDim.x) * blockDim.x) {
        bool empty;
        bad |= !row_offsets_sound<kCooTile>(g.ro, (u32)r, g.rows, base, g.nnz, 0u, nullptr, &empty);
    }
    // the ids need no rows: the entries [base, base + nnz) -- the place every call of the family reads a matrix from,
    // whatever its other offsets say -- in one streaming pass (first form: the row walk of the expansion, 3.4 ms for the
    // 52.6 M entries of the webbase product where the expansion itself took 0.42 ms)
    if (g.col) {
        const u32* col = g.col + base;
        for (u64 i = u64(blockIdx.x) * blockDim.x + threadIdx.x; i < g.nnz; i += u64(gridDim.x) * blockDim.x) bad |= col[i] >= g.cols;
    }
    if (bad) g.st->invalid = 1;
}

template <typename I>
__global__ __launch_bounds__(256) void to_coo_expand_kernel(const ToCooArgs g)
{
    SPECK_POISON();
    if (g.st->invalid) return;  // (the verdict of to_coo_check_kernel: nothing below runs on offsets or ids it refused)
    const u32 lane = lane_id();
    const u64 wave = (u64(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const u64 nwaves = (u64(gridDim.x) * blockDim.x) >> 6;
    const u64 base = g.st->base;
    I* const row_out = static_cast<I*>(g.row_out);
    I* const col_out = static_cast<I*>(g.col_out);
    const u32* const col = g.col;
    for (u64 r0 = wave * 64; r0 < g.rows; r0 += nwaves * 64) {
        const u64 r = r0 + lane;
        u32 a = 0, b = 0;
        if (r < g.rows) a = g.ro[r], b = g.ro[r + 1];
        const u64 id0 = g.row_base + r0;
        walk_row_entries(a, b, [&](u64 j, u32 l) { row_out[j - base] = (I)(id0 + l); });
    }
    // the columns need no rows: widened in one streaming pass
    if (col_out)
        for (u64 i = u64(blockIdx.x) * blockDim.x + threadIdx.x; i < g.nnz; i += u64(gridDim.x) * blockDim.x) col_out[i] = (I)col[base + i];
}

int to_coo_run(CooScratch* sc, hipStream_t s, const speck_dcsr* A, u32 index_bytes, u64 row_base, void* d_row_out, void* d_col_out)
{
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    CooStatus* st = static_cast<CooStatus*>(sc->fixed.p);
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(CooStatus), s));
    const u32 rows = (u32)A->rows;
    const ToCooArgs g{A->row_offsets, d_col_out ? A->col_ids : nullptr, rows, (u32)A->cols, A->nnz, row_base, A->col_ids, A->data, d_row_out,
                      d_col_out, index_bytes, st};
    // (a lane per row, four waves per workgroup; where columns were asked for, enough workgroups for the pass over the entries)
    const dim3 grid(grid_of(std::max((u64(rows) + 255) / 256, d_col_out ? (A->nnz + kCooTile - 1) / kCooTile : 0), 8192));
    SPECK_LAUNCH(to_coo_check_kernel, grid, dim3(256), 0, s, g);
    if (index_bytes == 8) SPECK_LAUNCH(to_coo_expand_kernel<u64>, grid, dim3(256), 0, s, g);
    else SPECK_LAUNCH(to_coo_expand_kernel<u32>, grid, dim3(256), 0, s, g);
    // the ONE read-back of the call
    CooStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    return h.invalid ? SPECK_ERR_INVALID : SPECK_OK;
}

const char* const kToGuardNames[1] = {"to_coo status"};

int to_coo_impl(speck_config* cfg, const speck_dcsr* A, u32 index_bytes, u64 row_base, void* d_row_out, void* d_col_out)
{
    if (!A || !d_row_out) return SPECK_ERR_INVALID;
    if (index_bytes != 4 && index_bytes != 8) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if ((A->rows && !A->row_offsets) || (A->nnz && (A->rows == 0 || (d_col_out && !A->col_ids)))) return SPECK_ERR_INVALID;
    // the last row index fits the index type: a u32, or an int64_t
    const u64 id_limit = index_bytes == 4 ? (1ull << 32) : (1ull << 63);
    if (row_base > id_limit || A->rows > id_limit - row_base) return SPECK_ERR_INVALID;
    // the outputs against each other and against what of A the host knows the place of (its entries: the check kernel)
    const u64 out_len = A->nnz * index_bytes;
    if (is_one_of(d_row_out, A) || (d_col_out && is_one_of(d_col_out, A))) return SPECK_ERR_INVALID;
    if (d_col_out && spans_overlap(d_row_out, out_len, d_col_out, out_len)) return SPECK_ERR_INVALID;
    if (spans_overlap(d_row_out, out_len, A->row_offsets, (A->rows + 1) * 4) ||
        spans_overlap(d_col_out, out_len, A->row_offsets, (A->rows + 1) * 4))
        return SPECK_ERR_INVALID;
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0) return SPECK_OK;  // no row, no entry: nothing to write

    CooScratch own;
    CooScratch* sc = cfg ? coo_scratch(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    int rc = to_coo_run(sc, s, A, index_bytes, row_base, d_row_out, d_col_out);
    if (rc != SPECK_OK) (void)hipStreamSynchronize(s);
    const void* whole[] = {sc->fixed.p};
    rc = guard_check_buffers(whole, kToGuardNames, 1, s, " by the COO expansion", rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    return rc;
}

}  // namespace

extern "C" {

int speck_from_coo_f64(speck_config* cfg, const speck_dcoo* coo, speck_dcsr* C, speck_from_coo_info* info)
{
    return from_coo_impl<double>(cfg, coo, C, info);
}

int speck_from_coo_f32(speck_config* cfg, const speck_dcoo* coo, speck_dcsr* C, speck_from_coo_info* info)
{
    return from_coo_impl<float>(cfg, coo, C, info);
}

int speck_to_coo(speck_config* cfg, const speck_dcsr* A, uint32_t index_bytes, uint64_t row_base, void* d_row_out, void* d_col_out)
{
    return to_coo_impl(cfg, A, index_bytes, row_base, d_row_out, d_col_out);
}

}  // extern "C"
