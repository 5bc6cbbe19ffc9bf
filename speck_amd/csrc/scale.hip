// scale.hip -- speck_scale_*: C(i,j) = ((alpha g(A(i,j))) (* or /) l[i]) (* or /) r[j] on the pattern of a device CSR, in
// place or into a new C; g is the identity, |v|, v v or 1.  Every step in double, one rounding to T.  The one map from a
// device vector back into a matrix (reduce.hip is the way out).  The reference has no counterpart.
//
//   scale_check_kernel    (scale.hpp: sddmm.hip queues it too) two kinds of workgroups in one launch.  A thread per row: the offsets ascend, stay inside
//                         [row_offsets[0], row_offsets[0] + nnz] and the last one spans nnz (entry_tiles.hpp, the check the
//                         reduction makes); with a row vector a row also tells every entry tile the rows of its first and
//                         last entry.  Where col_ids is read at all (a column vector, or a new C): a stream over the ids,
//                         each < cols.  Raises the verdict in the status block.
//   scale_stream_kernel   WITHOUT a row vector, queued behind it, looks at the verdict first.  Nothing here knows of rows: a
//                         lane takes a 16-byte chunk of `data` per step (and the chunk of col_ids beside it where a column
//                         vector or C asks), kSteps chunks in flight, a grid-stride loop.  Chunks lie at absolute 16-byte
//                         positions; the entries in front of the first and behind the last whole chunk go one by one.
//   scale_tile_kernel     WITH a row vector, one path for every row length.  A workgroup per ENTRY TILE: the absolute entries
//                         [4096 t, 4096 (t + 1)), clipped to the matrix; a thread holds 16 consecutive ones (16-byte loads
//                         and stores).  The rows that start in the tile AND hold an entry leave their number at their first
//                         entry's place in LDS and a bit in a bitmap; a thread learns the row of its first entry from the
//                         last such place in front of it (a max-scan over the threads; none: the row of the tile's first
//                         entry, which the checking pass left), then walks its 16 bits.  Rows without entries mark nothing,
//                         so thousands of them between two tiles, a tile inside one row and a tile of 4096 rows are one
//                         case.  l[i] is loaded where the row changes, not per entry.  Two forms: with the column ids
//                         (a column vector, a new C) and without (none held in registers: one more wave per SIMD).
//   scale_offsets_kernel  (scale.hpp) a new C only: its row offsets, rebased to 0.
// Every entry is written once by one thread; `nonfinite` is an integer counter (one atomic per workgroup).  No kernel
// uses scratch.  The host side is the side operations' own (side_call.hpp, compact.hpp: C by the multiply's rule).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "compact.hpp"
#include "entry_tiles.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scale.hpp"
#include "side_call.hpp"

// every product, square and quotient is rounded to double on its own, as numpy rounds them
#pragma clang fp contract(off)

using namespace speck;

namespace {

constexpr u32 kTile = SPECK_SCALE_TILE_ENTRIES, kThreads = 256, kPer = kTile / kThreads;
static_assert(kPer == 16, "a thread's row-start bits are half a word of the bitmap");
static_assert(kTile == kScaleTile && kThreads == kScaleThreads, "the checking pass of scale.hpp");
constexpr u32 kSteps = 4;            // 16-byte chunks a lane of the stream has in flight
constexpr u32 kStreamBlocks = 2048;  // ... and its grid at most (8 workgroups per CU; it strides over the rest)

template <typename T>
struct ScaleArgs {
    const u32* ro;
    const u32* col;  // read where a column vector or C asks
    const T* src;
    T* dst;        // in place: src, entry p at p; C's values otherwise, entry p at p - row_offsets[0]
    u32* dst_col;  // C's column ids (null: in place)
    const double *l, *r;
    u64 nnz;
    u32 rows, cols, map, row_mode, col_mode;
    u32 aligned;  // every array above that is read or written starts on a 16-byte boundary
    double alpha;
    const u32* tile_rows;
    ScaleStatus* st;
};

template <typename V, u32 N>
struct alignas(N * sizeof(V)) Vec {
    V v[N];
};

// one entry: the chain of the contract.  The branches are uniform (kernel arguments).
template <typename T>
__device__ __forceinline__ T scaled_entry(const ScaleArgs<T>& g, T a, double l, u32 c, u32& nonfinite)
{
#pragma clang fp contract(off)
    double x = (double)a;
    if (g.map == SPECK_MAP_ABS) x = __builtin_fabs(x);
    else if (g.map == SPECK_MAP_SQUARE) x = x * x;
    else if (g.map == SPECK_MAP_ONE) x = 1.0;
    x = g.alpha * x;
    if (g.row_mode == SPECK_SCALE_MUL) x = x * l;
    else if (g.row_mode == SPECK_SCALE_DIV) x = x / l;
    if (g.col_mode == SPECK_SCALE_MUL) x = x * g.r[c];
    else if (g.col_mode == SPECK_SCALE_DIV) x = x / g.r[c];
    const T y = (T)x;
    nonfinite += !__builtin_isfinite(y);
    return y;
}

// ------------------------------------------------------------------------------------------------ no row vector
// The entries [base, base + nnz) in chunks of N at absolute positions that are multiples of N (N = 1: entry by entry, where
// an array is not aligned for the wide form).  Returns the results this thread saw that are not finite.
template <typename T, u32 N>
__device__ __forceinline__ u32 stream_entries(const ScaleArgs<T>& g, u64 base, u64 d0, bool need_col)
{
    const u32 t = threadIdx.x;
    const u64 end = base + g.nnz;
    const u64 p0 = std::min<u64>((base + N - 1) / N * N, end), p1 = std::max<u64>(end / N * N, p0), nch = (p1 - p0) / N;
    const Vec<T, N>* src = reinterpret_cast<const Vec<T, N>*>(g.src + p0);
    const Vec<u32, N>* col = reinterpret_cast<const Vec<u32, N>*>(g.col + p0);
    Vec<T, N>* dst = reinterpret_cast<Vec<T, N>*>(g.dst + (p0 - d0));
    Vec<u32, N>* dst_col = reinterpret_cast<Vec<u32, N>*>(g.dst_col + (p0 - d0));
    u32 bad = 0;
    for (u64 cb = u64(blockIdx.x) * (kThreads * kSteps); cb < nch; cb += u64(gridDim.x) * (kThreads * kSteps)) {
        Vec<T, N> x[kSteps];
        Vec<u32, N> c[kSteps] = {};
#pragma unroll
        for (u32 u = 0; u < kSteps; ++u) {
            const u64 ch = cb + u * kThreads + t;
            if (ch < nch) {
                x[u] = src[ch];
                if (need_col) c[u] = col[ch];
            }
        }
#pragma unroll
        for (u32 u = 0; u < kSteps; ++u) {
            const u64 ch = cb + u * kThreads + t;
            if (ch < nch) {
#pragma unroll
                for (u32 j = 0; j < N; ++j) x[u].v[j] = scaled_entry(g, x[u].v[j], 1.0, c[u].v[j], bad);
                dst[ch] = x[u];
                if (g.dst_col) dst_col[ch] = c[u];
            }
        }
    }
    if (blockIdx.x == 0) {  // the entries in front of the first and behind the last whole chunk: fewer than 2 N
        const u64 nh = p0 - base, nt = end - p1;
        if (t < nh + nt) {
            const u64 p = t < nh ? base + t : p1 + (t - nh);
            const u32 c = need_col ? g.col[p] : 0u;
            g.dst[p - d0] = scaled_entry(g, g.src[p], 1.0, c, bad);
            if (g.dst_col) g.dst_col[p - d0] = c;
        }
    }
    return bad;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void scale_stream_kernel(const ScaleArgs<T> g)
{
    SPECK_POISON();
    __shared__ unsigned long long s_count;
    if (g.st->invalid) return;  // (the verdict of scale_check_kernel: nothing is written on input it refused)
    const u64 base = g.st->base, d0 = g.dst_col ? base : 0;
    const bool need_col = g.col_mode != SPECK_SCALE_NONE || g.dst_col;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    constexpr u32 N = 16 / sizeof(T);
    // (C's arrays count from A's first entry: the chunks of both sides coincide where that entry lies on a chunk's edge)
    const u32 bad = (g.aligned && d0 % N == 0) ? stream_entries<T, N>(g, base, d0, need_col) : stream_entries<T, 1>(g, base, d0, need_col);
    block_counter_to(&g.st->nonfinite, bad, &s_count);
}

// ------------------------------------------------------------------------------------------------ with a row vector
// kCols: col_ids is read (a column vector, or a new C).  A call without either holds no ids in registers.
template <typename T, bool kCols>
__global__ __launch_bounds__(kThreads) void scale_tile_kernel(const ScaleArgs<T> g)
{
    SPECK_POISON();
    constexpr u32 N = 16 / sizeof(T);
    __shared__ u32 s_row[kTile];          // at the place of a row's first entry: the row
    __shared__ u32 s_bits[kTile / 32];    // ... and a bit there
    __shared__ u32 s_last[kThreads];      // one past the last such place among the entries of the threads up to t (0: none)
    __shared__ unsigned long long s_count;
    if (g.st->invalid) return;  // (the verdict of scale_check_kernel: nothing below runs on offsets it refused)
    const u32 t = threadIdx.x;
    const u64 base = g.st->base, end = base + g.nnz;
    const u64 tile0 = (base / kTile + blockIdx.x) * kTile;
    if (tile0 >= end) return;  // (the grid is sized without knowing the base)
    const u64 lo = std::max(tile0, base), hi = std::min(tile0 + kTile, end);
    const u64 d0 = g.dst_col ? base : 0;
    const bool wide = g.aligned && lo == tile0 && hi == tile0 + kTile && d0 % 4 == 0;

    // the thread's 16 entries and, where asked, their column ids
    T a[kPer];
    u32 c[kCols ? kPer : 1] = {};
    const u64 q0 = tile0 + u64(t) * kPer;
    if (wide) {
        const Vec<T, N>* src = reinterpret_cast<const Vec<T, N>*>(g.src + q0);
        Vec<T, N> x[kPer / N];
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) x[k] = src[k];
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) a[k] = x[k / N].v[k % N];
        if (kCols) {
            const Vec<u32, 4>* cs = reinterpret_cast<const Vec<u32, 4>*>(g.col + q0);
            Vec<u32, 4> y[kPer / 4];
#pragma unroll
            for (u32 k = 0; k < kPer / 4; ++k) y[k] = cs[k];
#pragma unroll
            for (u32 k = 0; k < kPer; ++k) c[k] = y[k / 4].v[k % 4];
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            const bool in = p >= lo && p < hi;
            a[k] = in ? g.src[p] : T(0);
            if (kCols && in) c[k] = g.col[p];
        }
    }

    // the rows of the tile's first and last entry (scale_check_kernel); every row between them that holds an entry and
    // starts in the tile marks its first entry's place
    if (t < kTile / 32) s_bits[t] = 0;
    if (t == 0) s_count = 0;
    const u32 r_lo = std::min(g.tile_rows[2 * blockIdx.x], g.rows - 1u), r_hi = std::min(g.tile_rows[2 * blockIdx.x + 1], g.rows - 1u);
    __syncthreads();
    for (u64 r = u64(r_lo) + t; r <= r_hi; r += kThreads) {
        const u64 o = g.ro[r], e = g.ro[r + 1];
        if (o < e && o >= tile0 && o < tile0 + kTile) {
            const u32 i = (u32)(o - tile0);
            s_row[i] = (u32)r;
            atomicOr(&s_bits[i >> 5], 1u << (i & 31u));
        }
    }
    __syncthreads();

    // the row of the thread's first entry: the last marked place in front of it, across the threads
    const u32 bits = (s_bits[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu;
    const u32 mine = bits ? t * kPer + (31u - (u32)__clz((int)bits)) + 1u : 0u;
    s_last[t] = wave_inclusive_max(mine);
    __syncthreads();
    u32 before = (t & 63u) ? s_last[t - 1u] : 0u;
    for (u32 w = 0; w < (t >> 6); ++w) before = max(before, s_last[w * 64u + 63u]);
    u32 cur = before ? s_row[before - 1u] : r_lo;  // (none: the row that holds the tile's first entry)
    double l = g.l[cur];

    u32 bad = 0;
#pragma unroll
    for (u32 k = 0; k < kPer; ++k) {
        if ((bits >> k) & 1u) {
            cur = s_row[t * kPer + k];
            l = g.l[cur];
        }
        if (wide || (q0 + k >= lo && q0 + k < hi)) a[k] = scaled_entry(g, a[k], l, c[kCols ? k : 0], bad);
    }

    if (wide) {
        Vec<T, N>* dst = reinterpret_cast<Vec<T, N>*>(g.dst + (q0 - d0));
#pragma unroll
        for (u32 k = 0; k < kPer / N; ++k) {
            Vec<T, N> x;
#pragma unroll
            for (u32 j = 0; j < N; ++j) x.v[j] = a[k * N + j];
            dst[k] = x;
        }
        if (kCols && g.dst_col) {
            Vec<u32, 4>* dc = reinterpret_cast<Vec<u32, 4>*>(g.dst_col + (q0 - d0));
#pragma unroll
            for (u32 k = 0; k < kPer / 4; ++k) {
                Vec<u32, 4> y;
#pragma unroll
                for (u32 j = 0; j < 4; ++j) y.v[j] = c[k * 4 + j];
                dc[k] = y;
            }
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < kPer; ++k) {
            const u64 p = q0 + k;
            if (p >= lo && p < hi) {
                g.dst[p - d0] = a[k];
                if (kCols && g.dst_col) g.dst_col[p - d0] = c[k];
            }
        }
    }
    block_counter_to(&g.st->nonfinite, bad, &s_count);
}

// ------------------------------------------------------------------------------------------------ host
template <typename T>
int scale_run(ScaleScratch* sc, hipStream_t s, const speck_dcsr* A, const speck_scale_params* p, speck_dcsr* C,
              speck_scale_info* info, COut* out)
{
    const u32 rows = (u32)A->rows;
    const u64 nnz = A->nnz;
    if (rows == 0) return C ? publish_empty_c(C, A->cols, sizeof(T), s, out) : SPECK_OK;
    const bool tiled = p->row_mode != SPECK_SCALE_NONE, need_col = p->col_mode != SPECK_SCALE_NONE || C;
    const u32 max_tiles = tiled ? entry_tiles_at_most(nnz, kTile) : 0u;
    static_assert(sizeof(ScaleStatus) <= 256, "status block");
    int rc = sc->fixed.ensure(256);
    if (rc != SPECK_OK) return rc;
    if (max_tiles) {
        rc = sc->var.ensure(up256(size_t(max_tiles) * 8));
        if (rc != SPECK_OK) return rc;
    }
    // (nnz(C) = nnz(A) is known before the first kernel: C's buffers are taken now and handed over behind the verdict)
    if (C) {
        rc = prepare_c(C, rows, nnz, sizeof(T), out);
        if (rc != SPECK_OK) return rc;
    }
    ScaleStatus* st = static_cast<ScaleStatus*>(sc->fixed.p);
    u32* tile_rows = max_tiles ? static_cast<u32*>(sc->var.p) : nullptr;

    HIP_TRY(hipMemsetAsync(st, 0, sizeof(ScaleStatus), s));
    launch_scale_check(s, A, need_col, max_tiles, tile_rows, st);
    if (nnz) {
        T* dst = C ? static_cast<T*>(out->val) : static_cast<T*>(A->data);
        const bool aligned = on_16_bytes(A->data) && (!need_col || on_16_bytes(A->col_ids)) && on_16_bytes(dst) &&
                             (!C || on_16_bytes(out->col));
        const ScaleArgs<T> g{A->row_offsets, A->col_ids, static_cast<const T*>(A->data), dst, C ? out->col : nullptr,
                             p->d_row, p->d_col, nnz, rows, (u32)A->cols, p->map, p->row_mode, p->col_mode, aligned ? 1u : 0u,
                             p->alpha, tile_rows, st};
        if (tiled && need_col) SPECK_LAUNCH((scale_tile_kernel<T, true>), dim3(max_tiles), dim3(kThreads), 0, s, g);
        else if (tiled) SPECK_LAUNCH((scale_tile_kernel<T, false>), dim3(max_tiles), dim3(kThreads), 0, s, g);
        else {
            const u64 chunks = nnz / (16 / sizeof(T)) + 1;
            SPECK_LAUNCH(scale_stream_kernel<T>, dim3(grid_of((chunks + kThreads * kSteps - 1) / (kThreads * kSteps), kStreamBlocks)),
                         dim3(kThreads), 0, s, g);
        }
    }
    if (C) launch_scale_offsets(s, A, out->ro, st);
    // the ONE read-back of the call: the verdict, the base, the counter
    ScaleStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    if (C) publish_c(C, rows, A->cols, nnz, out);
    if (info) {
        info->entries = nnz;
        info->nonfinite = h.nonfinite;
        info->tiles = tiled && nnz ? (u64(h.base) + nnz - 1) / kTile - u64(h.base) / kTile + 1 : 0;
    }
    return SPECK_OK;
}

const char* const kGuardNamesC[5] = {"scale status", "scale tile rows", "C.data", "C.col_ids", "C.row_offsets"};
const char* const kGuardNamesA[5] = {"scale status", "scale tile rows", "A.data", "A.col_ids", "A.row_offsets"};

template <typename T>
int scale_impl(speck_config* cfg, const speck_dcsr* A, const speck_scale_params* p, speck_dcsr* C, speck_scale_info* info)
{
    if (!A || !p) return SPECK_ERR_INVALID;
    if (p->map > SPECK_MAP_ONE || p->row_mode > SPECK_SCALE_DIV || p->col_mode > SPECK_SCALE_DIV) return SPECK_ERR_INVALID;
    if ((p->row_mode != SPECK_SCALE_NONE) != (p->d_row != nullptr)) return SPECK_ERR_INVALID;
    if ((p->col_mode != SPECK_SCALE_NONE) != (p->d_col != nullptr)) return SPECK_ERR_INVALID;
    if (p->alpha != p->alpha) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27)) return SPECK_ERR_DIM_LIMIT;
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    // (col_ids is read only for a column vector or a new C: in place without one it may be NULL)
    const bool need_col = p->col_mode != SPECK_SCALE_NONE || C;
    if ((A->rows && !A->row_offsets) || (A->nnz && !A->data) || (A->rows == 0 && A->nnz)) return SPECK_ERR_INVALID;
    if (need_col && A->nnz && !A->col_ids) return SPECK_ERR_INVALID;
    for (const double* v : {p->d_row, p->d_col})
        if (v && (is_one_of(v, A) || (C && is_one_of(v, C)))) return SPECK_ERR_INVALID;
    if (C && shares_buffer(C, A)) return SPECK_ERR_INVALID;
    if (info) *info = speck_scale_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    return run_side_call(cfg, scale_scratch, C ? C : A, info, C ? kGuardNamesC : kGuardNamesA, " by the scaling",
                         [&](ScaleScratch* sc, hipStream_t s, COut* out) { return scale_run<T>(sc, s, A, p, C, info, out); });
}

}  // namespace

extern "C" {

int speck_scale_f64(speck_config* cfg, const speck_dcsr* A, const speck_scale_params* p, speck_dcsr* C, speck_scale_info* info)
{
    return scale_impl<double>(cfg, A, p, C, info);
}

int speck_scale_f32(speck_config* cfg, const speck_dcsr* A, const speck_scale_params* p, speck_dcsr* C, speck_scale_info* info)
{
    return scale_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
