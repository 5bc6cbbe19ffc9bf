// reduce.hip -- speck_reduce_*: per row and over all entries of a device CSR, the sum of v, |v| or v v, or the largest v,
// smallest v or largest |v|, in double.  Reads row_offsets and data, never col_ids.  The reference has no counterpart.
//
//   reduce_check_kernel    a thread per row: the offsets ascend, stay inside [row_offsets[0], row_offsets[0] + nnz] and the
//                          last one spans nnz; counts the rows without an entry.  Raises the verdict in the status block.
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
// The host side stands on host_common.hpp and side_call.hpp (the status read-back); the frame of the call is its own, as
// the row sort's is: no C is handed over.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "entry_tiles.hpp"
#include "launch.hpp"
#include "reduce.hpp"
#include "row_tiles.hpp"
#include "side_call.hpp"

// every square and every sum is rounded on its own: all code paths add the same terms (add.hip does the same per function)
#pragma clang fp contract(off)

using namespace speck;

namespace {

constexpr u32 kTile = SPECK_REDUCE_TILE_ENTRIES, kThreads = 256, kPer = SPECK_REDUCE_THREAD_ENTRIES, kWaves = kThreads / 64;
static_assert(kThreads * kPer == kTile && kPer == 16, "a thread's boundary bits are half a word of the bitmap");

struct ReduceStatus {
    u32 invalid;  // the offsets
    u32 base;     // row_offsets[0]
    unsigned long long rows_empty, rows_split;
    double total;
};

// what a tile leaves for the rows it does not hold whole, and its own total
struct TileRec {
    double head;   // the entries in front of the first row start (the row ends here), or the whole tile where it lies inside one row
    double tail;   // the entries from the last row start on, where that row goes on behind the tile
    double total;
    u32 tail_row, tail_end;  // that row and where it ends
    u32 chain;               // the row of `tail` starts in this tile: its result is combined from here
    u32 pad_;
};

template <int OP>
struct Op {
    static constexpr bool kSum = OP == SPECK_REDUCE_SUM || OP == SPECK_REDUCE_ABS_SUM || OP == SPECK_REDUCE_SQ_SUM;
    __host__ __device__ static double ident()
    {
        return OP == SPECK_REDUCE_MAX ? -__builtin_huge_val() : OP == SPECK_REDUCE_MIN ? __builtin_huge_val() : 0.0;
    }
    __device__ __forceinline__ static double term(double v)
    {
#pragma clang fp contract(off)
        if (OP == SPECK_REDUCE_ABS_SUM || OP == SPECK_REDUCE_ABS_MAX) return __builtin_fabs(v);
        if (OP == SPECK_REDUCE_SQ_SUM) return v * v;
        return v;
    }
    // (a NaN on either side comes out: `fmax` would drop it)
    __device__ __forceinline__ static double comb(double a, double b)
    {
#pragma clang fp contract(off)
        if (kSum) return a + b;
        if (OP == SPECK_REDUCE_MIN) return (a < b || a != a) ? a : b;
        return (a > b || a != a) ? a : b;
    }
};

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_move_f64(double old, double v)
{
    const u64 o = (u64)__double_as_longlong(old), x = (u64)__double_as_longlong(v);
    const u32 lo = dpp_move<CTRL, ROW_MASK>((u32)o, (u32)x), hi = dpp_move<CTRL, ROW_MASK>((u32)(o >> 32), (u32)(x >> 32));
    return __longlong_as_double((long long)((u64(hi) << 32) | lo));
}

// one step of the segmented inclusive scan: x = the combination of the lanes of my segment up to me, f = "a segment
// starts in a lane up to me".  Lanes without a source receive the identity.
template <typename O, int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ void segmented_step(double& x, u32& f)
{
    const double px = dpp_move_f64<CTRL, ROW_MASK>(O::ident(), x);
    const u32 pf = dpp_move<CTRL, ROW_MASK>(0u, f);
    x = f ? x : O::comb(px, x);
    f |= pf;
}

template <typename O>
__device__ __forceinline__ void wave_segmented_scan(double& x, u32& f)
{
    segmented_step<O, kDppRowShr + 1>(x, f);
    segmented_step<O, kDppRowShr + 2>(x, f);
    segmented_step<O, kDppRowShr + 4>(x, f);
    segmented_step<O, kDppRowShr + 8>(x, f);
    segmented_step<O, kDppRowBcast15, 0xA>(x, f);
    segmented_step<O, kDppRowBcast31, 0xC>(x, f);
}

// all 64 lanes combined, a fixed butterfly (lane 0's result is what is used)
template <typename O>
__device__ __forceinline__ double wave_combine(double x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = O::comb(x, __shfl_xor(x, m));
    return x;
}

// ------------------------------------------------------------------------------------------------ check
// tile_rows[2 i], [2 i + 1]: the rows of the first and of the last entry of the i-th tile the matrix touches
__global__ __launch_bounds__(kThreads) void reduce_check_kernel(const u32* __restrict__ ro, u32 rows, u64 nnz, u32 max_tiles,
                                                                u32* __restrict__ tile_rows, ReduceStatus* st)
{
    SPECK_POISON();
    __shared__ unsigned long long s_empty;
    const u32 r = blockIdx.x * kThreads + threadIdx.x;
    const u32 base = ro[0];
    if (threadIdx.x == 0) s_empty = 0;
    if (r == 0) st->base = base;
    __syncthreads();
    bool empty = false;
    if (r < rows && !row_offsets_sound<kTile>(ro, r, rows, base, nnz, max_tiles, tile_rows, &empty)) st->invalid = 1;
    block_counter_to(&st->rows_empty, (u32)empty, &s_empty);
}

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

template <typename T>
struct alignas(16) Vec16 {
    T v[16 / sizeof(T)];
};

// where the running value at entry i of the tile rests in LDS (a thread's 16 entries 17 doubles apart: two lanes per bank)
__device__ __forceinline__ u32 val_slot(u32 i) { return i + (i >> 4); }

template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void reduce_tile_kernel(const ReduceArgs<T> g)
{
    SPECK_POISON();
    using O = Op<OP>;
    __shared__ double s_val[kTile + kTile / 16];
    __shared__ double s_incl[kThreads];
    __shared__ double s_wave[kWaves], s_wtot[kWaves];
    __shared__ u32 s_wflag[kWaves];
    __shared__ u32 s_bits[kTile / 32];
    if (g.st->invalid) return;  // (the verdict of reduce_check_kernel: nothing below runs on offsets it refused)
    const u32 t = threadIdx.x, lane = lane_id(), wid = t >> 6;
    const u64 base = g.st->base, end = base + g.nnz;
    const u64 tile0 = (base / kTile + blockIdx.x) * kTile;
    if (tile0 >= end) return;  // (the grid is sized without knowing the base)
    const u64 lo = std::max(tile0, base), hi = std::min(tile0 + kTile, end);

    // the thread's 16 entries: their terms, the identity where the matrix does not reach
    double v[kPer];
    const u64 q0 = tile0 + u64(t) * kPer;
    if (lo == tile0 && hi == tile0 + kTile) {
        constexpr u32 N = 16 / sizeof(T);
        const Vec16<T>* src = reinterpret_cast<const Vec16<T>*>(g.data + q0);
        Vec16<T> x[kPer / N];
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) x[k] = src[k];
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) v[k] = O::term((double)x[k / N].v[k % N]);
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            v[k] = (p >= lo && p < hi) ? O::term((double)g.data[p]) : O::ident();
        }
    }

    // the rows of the tile's first and last entry (reduce_check_kernel), and the row starts inside the tile as a bitmap
    if (t < kTile / 32) s_bits[t] = 0;
    const u32 r_lo = g.tile_rows[2 * blockIdx.x], r_hi = g.tile_rows[2 * blockIdx.x + 1];
    __syncthreads();
    for (u64 r = u64(r_lo) + t; r <= u64(r_hi) + 1; r += kThreads) {
        const u64 o = g.ro[r];
        if (o >= tile0 && o < tile0 + kTile) atomicOr(&s_bits[(u32)(o - tile0) >> 5], 1u << ((u32)(o - tile0) & 31u));
    }
    __syncthreads();

    // in the thread: the running value restarts at every row start; what it was in front of one, and at the thread's
    // last entry, goes to LDS
    const u32 bits = (s_bits[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu;
    double acc = O::ident(), tot = O::ident();
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        if ((bits >> k) & 1u) {
            if (k) s_val[val_slot(t * kPer + k - 1u)] = acc;
            acc = O::ident();
        }
        acc = O::comb(acc, v[k]);
        tot = O::comb(tot, v[k]);
    }
    s_val[val_slot(t * kPer + kPer - 1u)] = acc;

    // across the threads: segmented by "a row starts in this thread"
    double x = acc;
    u32 f = bits != 0;
    wave_segmented_scan<O>(x, f);
    tot = wave_combine<O>(tot);
    if (lane == 63) s_wave[wid] = x, s_wflag[wid] = f;
    if (lane == 0) s_wtot[wid] = tot;
    __syncthreads();
    double carry = O::ident();
    for (u32 u = 0; u < wid; ++u) carry = s_wflag[u] ? s_wave[u] : O::comb(carry, s_wave[u]);
    s_incl[t] = f ? x : O::comb(carry, x);
    __syncthreads();

    // the rows that end in the tile (rows without entries: reduce_finish_kernel)
    TileRec* rec = g.recs + blockIdx.x;
    for (u64 r = u64(r_lo) + t; r <= r_hi; r += kThreads) {
        const u64 s = g.ro[r], e = g.ro[r + 1];
        if (s == e || e > hi) continue;  // (e > lo: r >= r_lo)
        const u32 le = (u32)(e - 1 - tile0), te = le >> 4;
        double val = s_val[val_slot(le)];
        if (s < tile0 + u64(te) * kPer) val = O::comb(te ? s_incl[te - 1u] : O::ident(), val);
        if (s < lo) rec->head = val;
        else if (g.row_out) g.row_out[r] = val;
    }
    if (t == 0) {
        const u64 s_first = g.ro[r_lo], e_last = g.ro[r_hi + 1u];
        const bool head = s_first < lo, tail = e_last > hi, whole = head && tail && r_lo == r_hi;
        if (whole) rec->head = s_incl[kThreads - 1u];
        rec->tail = s_incl[kThreads - 1u];
        rec->tail_row = r_hi;
        rec->tail_end = (u32)e_last;
        rec->chain = tail && !whole;
        double total = s_wtot[0];
        for (u32 u = 1; u < kWaves; ++u) total = O::comb(total, s_wtot[u]);
        rec->total = total;
    }
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
    const u64 base = st->base, t_first = base / kTile;
    const u32 ntiles = nnz ? (u32)((base + nnz - 1) / kTile - t_first + 1) : 0u;
    if (blockIdx.x < chain_blocks) {
        // a wave per tile: the row that leaves it open = its tail, the whole tiles inside the row (a lane takes every
        // 64th, then the butterfly), the head of the tile it ends in
        const u32 i = blockIdx.x * kWaves + wid;
        if (i >= ntiles || !recs[i].chain) return;
        const u32 ib = (u32)((u64(recs[i].tail_end) - 1) / kTile - t_first);
        double mid = O::ident();
        for (u32 j = i + 1u + lane; j < ib; j += 64u) mid = O::comb(mid, recs[j].head);
        mid = wave_combine<O>(mid);
        const double val = O::comb(O::comb(recs[i].tail, mid), recs[ib].head);
        if (lane == 0 && row_out) row_out[recs[i].tail_row] = val;
    } else if (blockIdx.x < chain_blocks + row_blocks) {
        const u32 r = (blockIdx.x - chain_blocks) * kThreads + t;
        if (row_out && r < rows && ro[r] == ro[r + 1]) row_out[r] = O::ident();
    } else {
        double acc = O::ident();
        u32 split = 0;  // (one atomic per split row on one word of global memory was the longest thing in the call)
        for (u32 j = t; j < ntiles; j += kThreads) acc = O::comb(acc, recs[j].total), split += recs[j].chain;
        acc = wave_combine<O>(acc);
        split = wave_reduce_add(split);
        if (lane == 0) s_w[wid] = acc, s_split[wid] = split;
        __syncthreads();
        if (t == 0) {
            double total = s_w[0];
            for (u32 u = 1; u < kWaves; ++u) total = O::comb(total, s_w[u]), split += s_split[u];
            st->total = total;
            st->rows_split = split;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, int OP>
void reduce_launch(hipStream_t s, const speck_dcsr* A, double* d_row_out, u32 max_tiles, TileRec* recs, const u32* tile_rows,
                   ReduceStatus* st)
{
    const u32 rows = (u32)A->rows;
    if (max_tiles) {
        const ReduceArgs<T> g{A->row_offsets, static_cast<const T*>(A->data), rows, A->nnz, d_row_out, recs, tile_rows, st};
        SPECK_LAUNCH((reduce_tile_kernel<T, OP>), dim3(max_tiles), dim3(kThreads), 0, s, g);
    }
    const u32 chain_blocks = (max_tiles + kWaves - 1) / kWaves, row_blocks = (rows + kThreads - 1) / kThreads;
    SPECK_LAUNCH(reduce_finish_kernel<OP>, dim3(chain_blocks + row_blocks + 1u), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 chain_blocks, row_blocks, d_row_out, recs, st);
}

double identity_of(int op)
{
    return op == SPECK_REDUCE_MAX ? Op<SPECK_REDUCE_MAX>::ident() : op == SPECK_REDUCE_MIN ? Op<SPECK_REDUCE_MIN>::ident() : 0.0;
}

template <typename T>
int reduce_run(ReduceScratch* sc, hipStream_t s, const speck_dcsr* A, int op, double* d_row_out, ReduceStatus* h)
{
    const u32 max_tiles = entry_tiles_at_most(A->nnz, kTile);
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    const size_t rec_bytes = up256(size_t(std::max(max_tiles, 1u)) * sizeof(TileRec));
    rc = sc->var.ensure(rec_bytes + up256(size_t(std::max(max_tiles, 1u)) * 8));
    if (rc != SPECK_OK) return rc;
    static_assert(sizeof(ReduceStatus) <= 256, "status block");
    ReduceStatus* st = static_cast<ReduceStatus*>(sc->fixed.p);
    TileRec* recs = static_cast<TileRec*>(sc->var.p);
    u32* tile_rows = reinterpret_cast<u32*>(static_cast<unsigned char*>(sc->var.p) + rec_bytes);

    HIP_TRY(hipMemsetAsync(st, 0, sizeof(ReduceStatus), s));
    const u32 rows = (u32)A->rows;
    SPECK_LAUNCH(reduce_check_kernel, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0, s, A->row_offsets, rows, A->nnz,
                 max_tiles, tile_rows, st);
    switch (op) {
    case SPECK_REDUCE_SUM: reduce_launch<T, SPECK_REDUCE_SUM>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    case SPECK_REDUCE_ABS_SUM: reduce_launch<T, SPECK_REDUCE_ABS_SUM>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    case SPECK_REDUCE_SQ_SUM: reduce_launch<T, SPECK_REDUCE_SQ_SUM>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    case SPECK_REDUCE_MAX: reduce_launch<T, SPECK_REDUCE_MAX>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    case SPECK_REDUCE_MIN: reduce_launch<T, SPECK_REDUCE_MIN>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    default: reduce_launch<T, SPECK_REDUCE_ABS_MAX>(s, A, d_row_out, max_tiles, recs, tile_rows, st); break;
    }
    // the ONE read-back of the call: the verdict, the counters, the total
    rc = read_status(s, st, h);
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
    if (d_row_out && (d_row_out == A->data || (void*)d_row_out == (void*)A->col_ids || (void*)d_row_out == (void*)A->row_offsets))
        return SPECK_ERR_INVALID;
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    if (A->rows == 0) {  // no row, no entry: the identity
        if (h_total) *h_total = identity_of(op);
        if (info) *info = speck_reduce_info{};
        return SPECK_OK;
    }
    ReduceScratch own;
    ReduceScratch* sc = cfg ? reduce_scratch(cfg) : &own;
    const hipStream_t s = cfg ? call_stream(cfg) : nullptr;
    (void)take_launch_error();
    ReduceStatus h{};
    int rc = reduce_run<T>(sc, s, A, op, d_row_out, &h);
    if (rc != SPECK_OK) (void)hipStreamSynchronize(s);
    const void* whole[] = {sc->fixed.p, sc->var.p};
    rc = guard_check_buffers(whole, kGuardNames, 2, s, " by the reduction", rc);
    if (!cfg) {
        (void)hipStreamSynchronize(s);
        own.release();
    }
    if (rc != SPECK_OK) {
        if (info) *info = speck_reduce_info{};
        return rc;
    }
    if (h_total) *h_total = h.total;
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

int speck_reduce_f64(speck_config* cfg, const speck_dcsr* A, int op, double* d_row_out, double* h_total, speck_reduce_info* info)
{
    return reduce_impl<double>(cfg, A, op, d_row_out, h_total, info);
}

int speck_reduce_f32(speck_config* cfg, const speck_dcsr* A, int op, double* d_row_out, double* h_total, speck_reduce_info* info)
{
    return reduce_impl<float>(cfg, A, op, d_row_out, h_total, info);
}

}  // extern "C"
