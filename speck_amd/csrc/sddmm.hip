// sddmm.hip -- speck_sddmm_*: C(i,j) = alpha sum_c U(i,c) V(j,c) (+ beta A(i,j), or times A(i,j)) on the pattern of a device
// CSR, in place or into a new C; U (rows x k) and V (cols x k) row-major device arrays of doubles.  The one map (block,
// block) -> matrix: the reduction runs over k, ACROSS THE LANES of a group, not over the entries of a row, so nothing
// here is tile_combine.hpp's.  Every step in double, one rounding to T.  The reference has no counterpart.
//
//   scale_check_kernel    (scale.hpp, the scaling's own) two kinds of workgroups in one launch.  A thread per row: the
//                         offsets (entry_tiles.hpp), and the rows of every entry tile's first and last entry.  A stream
//                         over col_ids: each < cols (compared, never followed).  Raises the verdict in the status block.
//   sddmm_tile_kernel     queued behind it, looks at the verdict first.  A workgroup per ENTRY TILE of 4096 absolute
//                         entries.  Phase A, a thread per 16 consecutive entries: the ids (16-byte loads where aligned),
//                         the row of each entry as scale_tile_kernel finds it (row-start bitmap, a max-scan, tile_rows for
//                         the tile's first entry); (row, id) of the 4096 entries stay in LDS; a new C gets its ids here.
//                         Phase B, a group of L = L(k) lanes per entry, the 256 / L groups of the workgroup side by side
//                         over the tile, kFlight entries per group in flight: lane l takes the pairs of columns q = l,
//                         l + L, ... of U(i,:) and V(j,:) -- one 16-byte load per lane, row and trip where the block lies
//                         on 16 bytes and its ld is even, 8-byte loads elsewhere -- ALL loads of a round and trip are
//                         issued before the first term; the lane's partial sum in the order of the contract; the butterfly
//                         over the group (__shfl_xor).  Lane 0 of a group applies alpha / beta / mode, rounds to T and
//                         writes the entry directly (not staged through LDS for wide stores: not measured).  L <= 8:
//                         what an entry costs beside its loads -- the two LDS reads, the addresses, the butterfly --
//                         is paid by every lane of its group, and measured it outweighs the shorter chain of trips
//                         of a wider group from k = 8 on.  Two trips of loads in flight instead of one: 130 registers,
//                         three waves per SIMD instead of four, 0 to 16 % slower.
//   scale_offsets_kernel  (scale.hpp) a new C only: its row offsets, rebased to 0.
// Every entry is written once by one thread; `nonfinite` is an integer counter (one atomic per workgroup).  No kernel
// uses scratch.  The host side is the side operations' own (side_call.hpp, compact.hpp: C by the multiply's rule).
//
// speck_sddmm_*_b32: U and V in float (B = float below).  The same tiles, the same L(k), the same tree through the same
// kernel with the block type as a template parameter; an element is widened where its term is formed ((double)u *
// (double)v: exact), so C is bit for bit the doubles' result on widened blocks.  A lane's pair of columns is 8 bytes: one
// 8-byte load where the block lies on 8 bytes and its ld is even, 4-byte loads elsewhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "compact.hpp"
#include "entry_tiles.hpp"
#include "launch.hpp"
#include "row_tiles.hpp"
#include "scale.hpp"
#include "side_call.hpp"

// every product and every sum is rounded to double on its own
#pragma clang fp contract(off)

using namespace speck;

namespace {

constexpr u32 kTile = SPECK_SDDMM_TILE_ENTRIES, kThreads = 256, kPer = kTile / kThreads;
static_assert(kPer == 16, "a thread's row-start bits are half a word of the bitmap");
static_assert(kTile == kScaleTile && kThreads == kScaleThreads, "the checking pass of scale.hpp");
constexpr u32 kFlight = 4;  // entries a group has in flight

// L(k) of the contract (speck_c_api.h): min(8, max(1, pow2ceil(ceil(k / 4)))), set from measurement.
// (SPECK_SDDMM_FORCE_LANES: one L for every k, up to 64 -- measurement builds only, profiles/sddmm.txt)
#ifdef SPECK_SDDMM_FORCE_LANES
constexpr u32 kMaxLanes = 64;
inline u32 lanes_of(u32) { return SPECK_SDDMM_FORCE_LANES; }
#else
constexpr u32 kMaxLanes = 8;
inline u32 lanes_of(u32 k)
{
    u32 lanes = 1;
    while (lanes < kMaxLanes && 4 * lanes < k) lanes *= 2;
    return lanes;
}
#endif

template <typename T, typename B = double>
struct SddmmArgs {
    const u32* ro;
    const u32* col;  // null: k == 0 in place, nobody asks
    const T* src;    // read where need_a
    T* dst;          // in place: src, entry p at p; C's values otherwise, entry p at p - row_offsets[0]
    u32* dst_col;    // C's column ids (null: in place)
    const B *u, *v;
    u64 nnz, ldu, ldv;
    u32 rows, k, mode;
    u32 need_a;          // HADAMARD, or beta != 0
    u32 aligned;         // col (and dst_col) start on 16-byte boundaries
    u32 wide_u, wide_v;  // the block starts on a boundary of 2 sizeof(B) bytes and its ld is even: a pair of columns lies on one
    double alpha, beta;
    const u32* tile_rows;
    ScaleStatus* st;
};

template <typename V, u32 N>
struct alignas(N * sizeof(V)) Vec {
    V v[N];
};

// ------------------------------------------------------------------------------------------------ tiles
// the columns c, c + 1 of a row (`two`: c + 1 < k; the column behind the last one is never read)
template <typename B>
__device__ __forceinline__ void load_pair(const B* at, bool wide, bool two, B& x0, B& x1)
{
    if (wide && two) {
        const Vec<B, 2> p = *reinterpret_cast<const Vec<B, 2>*>(at);
        x0 = p.v[0], x1 = p.v[1];
    } else {
        x0 = at[0];
        x1 = two ? at[1] : B(0);
    }
}

// Phase B: the entries [e_lo, e_hi) of the tile, whose (row, id) stand in LDS.  Returns the results this thread wrote that
// are not finite.
template <typename T, u32 L, typename B>
__device__ __forceinline__ u32 dot_entries(const SddmmArgs<T, B>& g, const u32* s_row, const u32* s_id, u32 e_lo, u32 e_hi, u64 tile0,
                                           u64 d0)
{
#pragma clang fp contract(off)
    constexpr u32 G = kThreads / L;
    const u32 l = threadIdx.x % L, grp = threadIdx.x / L;
    const u32 k = g.k;
    const bool wide_u = g.wide_u, wide_v = g.wide_v;
    u32 bad = 0;
    for (u32 eb = e_lo; eb < e_hi; eb += G * kFlight) {
        u32 e[kFlight];
        const B *ur[kFlight], *vr[kFlight];
        double a[kFlight], p[kFlight];
#pragma unroll
        for (u32 f = 0; f < kFlight; ++f) {
            e[f] = eb + f * G + grp;
            // (a group behind the tile's last entry walks that of e_lo: loads of memory that exists, a result nobody writes)
            const u32 at = e[f] < e_hi ? e[f] : e_lo;
            ur[f] = g.u + u64(s_row[at]) * g.ldu;
            vr[f] = g.v + u64(s_id[at]) * g.ldv;
            a[f] = (g.need_a && l == 0 && e[f] < e_hi) ? (double)g.src[tile0 + e[f]] : 0.0;
            p[f] = 0.0;  // a lane that owns no column
        }
        // lane l: the pairs q = l, l + L, ...; all loads of a trip before its terms; the first term seeds the sum
        auto trip = [&](u32 c, auto seeds) {
            const bool two = c + 1 < k;
            B x0[kFlight], x1[kFlight], y0[kFlight], y1[kFlight];
#pragma unroll
            for (u32 f = 0; f < kFlight; ++f) {
                load_pair(ur[f] + c, wide_u, two, x0[f], x1[f]);
                load_pair(vr[f] + c, wide_v, two, y0[f], y1[f]);
            }
#pragma unroll
            for (u32 f = 0; f < kFlight; ++f) {
                const double t0 = (double)x0[f] * (double)y0[f];
                p[f] = decltype(seeds)::value ? t0 : p[f] + t0;
                if (two) p[f] = p[f] + (double)x1[f] * (double)y1[f];
            }
        };
        u32 c = 2 * l;
        if (c < k) {
            trip(c, std::true_type{});
            for (c += 2 * L; c < k; c += 2 * L) trip(c, std::false_type{});
        }
        // the butterfly over the group: every lane ends with the same bits
#pragma unroll
        for (u32 s = L / 2; s; s >>= 1) {
#pragma unroll
            for (u32 f = 0; f < kFlight; ++f) p[f] = p[f] + __shfl_xor(p[f], (int)s, 64);
        }
#pragma unroll
        for (u32 f = 0; f < kFlight; ++f) {
            if (l == 0 && e[f] < e_hi) {
                double x = g.alpha * p[f];
                if (g.mode == SPECK_SDDMM_HADAMARD) x = x * a[f];
                else if (g.need_a) x = x + g.beta * a[f];
                const T y = (T)x;
                bad += !__builtin_isfinite(y);
                g.dst[tile0 + e[f] - d0] = y;
            }
        }
    }
    return bad;
}

template <typename T, u32 L, typename B>
__global__ __launch_bounds__(kThreads) void sddmm_tile_kernel(const SddmmArgs<T, B> g)
{
    SPECK_POISON();
    __shared__ u32 s_row[kTile];        // at the place of a row's first entry: the row; behind phase A: every entry's row
    __shared__ u32 s_id[kTile];         // every entry's column id
    __shared__ u32 s_bits[kTile / 32];  // a bit at the place of a row's first entry
    __shared__ u32 s_last[kThreads];    // one past the last such place among the entries of the threads up to t (0: none)
    __shared__ unsigned long long s_count;
    if (g.st->invalid) return;  // (the verdict of scale_check_kernel: nothing below runs on offsets or ids it refused)
    const u32 t = threadIdx.x;
    const u64 base = g.st->base, end = base + g.nnz;
    const u64 tile0 = (base / kTile + blockIdx.x) * kTile;
    if (tile0 >= end) return;  // (the grid is sized without knowing the base)
    const u64 lo = std::max(tile0, base), hi = std::min(tile0 + kTile, end);
    const u64 d0 = g.dst_col ? base : 0;
    const bool wide = g.aligned && lo == tile0 && hi == tile0 + kTile && d0 % 4 == 0;

    // the thread's 16 column ids; a new C takes them as they come
    u32 c[kPer] = {};
    const u64 q0 = tile0 + u64(t) * kPer;
    if (g.col) {
        if (wide) {
            const Vec<u32, 4>* cs = reinterpret_cast<const Vec<u32, 4>*>(g.col + q0);
            Vec<u32, 4> y[kPer / 4];
#pragma unroll
            for (u32 j = 0; j < kPer / 4; ++j) y[j] = cs[j];
            if (g.dst_col) {
                Vec<u32, 4>* dc = reinterpret_cast<Vec<u32, 4>*>(g.dst_col + (q0 - d0));
#pragma unroll
                for (u32 j = 0; j < kPer / 4; ++j) dc[j] = y[j];
            }
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) c[j] = y[j / 4].v[j % 4];
        } else {
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) {
                const u64 p = q0 + j;
                if (p >= lo && p < hi) {
                    c[j] = g.col[p];
                    if (g.dst_col) g.dst_col[p - d0] = c[j];
                }
            }
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
    u32 row[kPer];
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) {
        if ((bits >> j) & 1u) cur = s_row[t * kPer + j];
        row[j] = cur;
    }
    __syncthreads();  // (every thread has read the marks: the places take every entry's row now)
    {
        Vec<u32, 4>* sr = reinterpret_cast<Vec<u32, 4>*>(s_row + t * kPer);
        Vec<u32, 4>* si = reinterpret_cast<Vec<u32, 4>*>(s_id + t * kPer);
#pragma unroll
        for (u32 j = 0; j < kPer / 4; ++j) {
            Vec<u32, 4> a, b;
#pragma unroll
            for (u32 i = 0; i < 4; ++i) a.v[i] = row[j * 4 + i], b.v[i] = c[j * 4 + i];
            sr[j] = a, si[j] = b;
        }
    }
    __syncthreads();

    const u32 bad = dot_entries<T, L>(g, s_row, s_id, (u32)(lo - tile0), (u32)(hi - tile0), tile0, d0);
    block_counter_to(&g.st->nonfinite, bad, &s_count);
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, u32 L, typename B>
void launch_tiles(u32 lanes, u32 tiles, hipStream_t s, const SddmmArgs<T, B>& g)
{
    if (lanes == L) SPECK_LAUNCH((sddmm_tile_kernel<T, L, B>), dim3(tiles), dim3(kThreads), 0, s, g);
    else if constexpr (L < kMaxLanes) launch_tiles<T, 2 * L>(lanes, tiles, s, g);
}

// whether a pair of columns (c even) of a block lies on a boundary of its own size
template <typename B>
inline bool pair_aligned(const B* d, u64 ld)
{
    return reinterpret_cast<uintptr_t>(d) % (2 * sizeof(B)) == 0 && ld % 2 == 0;
}

// P: speck_sddmm_params or speck_sddmm_params_b32 (B: what its blocks hold)
template <typename T, typename P>
int sddmm_run(ScaleScratch* sc, hipStream_t s, const speck_dcsr* A, const P* p, speck_dcsr* C, speck_sddmm_info* info, COut* out)
{
    using B = std::remove_cv_t<std::remove_pointer_t<decltype(p->d_U)>>;
    const u32 rows = (u32)A->rows;
    const u64 nnz = A->nnz;
    if (rows == 0) return C ? publish_empty_c(C, A->cols, sizeof(T), s, out) : SPECK_OK;
    const bool need_col = p->k || C, need_a = p->mode == SPECK_SDDMM_HADAMARD || p->beta != 0.0;
    const u32 max_tiles = entry_tiles_at_most(nnz, kTile);
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
        const bool aligned = on_16_bytes(A->col_ids) && (!C || on_16_bytes(out->col));
        const SddmmArgs<T, B> g{A->row_offsets, need_col ? A->col_ids : nullptr, static_cast<const T*>(A->data), dst,
                                C ? out->col : nullptr, p->d_U, p->d_V, nnz, p->ldu, p->ldv, rows, p->k, p->mode, need_a ? 1u : 0u,
                                aligned ? 1u : 0u, pair_aligned(p->d_U, p->ldu) ? 1u : 0u, pair_aligned(p->d_V, p->ldv) ? 1u : 0u,
                                p->alpha, p->beta, tile_rows, st};
        launch_tiles<T, 1>(lanes_of(p->k), max_tiles, s, g);
    }
    if (C) launch_scale_offsets(s, A, out->ro, st);
    // the ONE read-back of the call: the verdict, the base, the counter
    ScaleStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    if (C) publish_c(C, rows, A->cols, nnz, out);
    if (info) {
        info->nonfinite = h.nonfinite;
        info->tiles = nnz ? (u64(h.base) + nnz - 1) / kTile - u64(h.base) / kTile + 1 : 0;
    }
    return SPECK_OK;
}

const char* const kGuardNamesC[5] = {"sddmm status", "sddmm tile rows", "C.data", "C.col_ids", "C.row_offsets"};
const char* const kGuardNamesA[5] = {"sddmm status", "sddmm tile rows", "A.data", "A.col_ids", "A.row_offsets"};

// whether the `elements` elements from v on hold one of X's three pointers
template <typename B>
bool span_holds_one_of(const B* v, u64 elements, const speck_dcsr* X)
{
    const u64 v0 = reinterpret_cast<uintptr_t>(v), bytes = sizeof(B) * elements;
    for (const void* q : {static_cast<const void*>(X->data), static_cast<const void*>(X->col_ids), static_cast<const void*>(X->row_offsets)})
        if (q && reinterpret_cast<uintptr_t>(q) - v0 < bytes) return true;  // (q < v0 wraps to more than any span)
    return false;
}

template <typename T, typename P>
int sddmm_impl(speck_config* cfg, const speck_dcsr* A, const P* p, speck_dcsr* C, speck_sddmm_info* info)
{
    if (!A || !p) return SPECK_ERR_INVALID;
    if (p->mode > SPECK_SDDMM_HADAMARD || p->alpha != p->alpha || p->beta != p->beta) return SPECK_ERR_INVALID;
    if (p->mode == SPECK_SDDMM_HADAMARD && p->beta != 0.0) return SPECK_ERR_INVALID;
    if (A->rows > (1ull << 27) || A->cols > (1ull << 27) || p->k > SPECK_SDDMM_MAX_K) return SPECK_ERR_DIM_LIMIT;
    if (p->ldu > (1ull << 32) || p->ldv > (1ull << 32)) return SPECK_ERR_DIM_LIMIT;  // (the spans below stay inside 64 bits)
    if (A->nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (p->ldu < p->k || p->ldv < p->k) return SPECK_ERR_INVALID;
    if (A->rows && !A->row_offsets) return SPECK_ERR_INVALID;
    // (entries without a row to hold them; entries without a column to point at: every id is >= cols)
    if (A->nnz && (A->rows == 0 || A->cols == 0)) return SPECK_ERR_INVALID;
    const bool need_a = p->mode == SPECK_SDDMM_HADAMARD || p->beta != 0.0;
    if (A->nnz && p->k && (!p->d_U || !p->d_V)) return SPECK_ERR_INVALID;
    if (A->nnz && (p->k || C) && !A->col_ids) return SPECK_ERR_INVALID;
    if (A->nnz && !A->data && (need_a || !C)) return SPECK_ERR_INVALID;
    // what the call may read of the blocks, padding inside included, holds nothing the call reads as A or writes
    if (p->k) {
        const decltype(p->d_U) blocks[2] = {p->d_U, p->d_V};
        const u64 spans[2] = {A->rows ? (A->rows - 1) * p->ldu + p->k : 0, A->cols ? (A->cols - 1) * p->ldv + p->k : 0};
        for (int b = 0; b < 2; ++b)
            if (blocks[b] && (span_holds_one_of(blocks[b], spans[b], A) || (C && span_holds_one_of(blocks[b], spans[b], C))))
                return SPECK_ERR_INVALID;
    }
    if (C && shares_buffer(C, A)) return SPECK_ERR_INVALID;
    if (info) *info = speck_sddmm_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    const int rc = run_side_call(cfg, sddmm_scratch, C ? C : A, info, C ? kGuardNamesC : kGuardNamesA, " by the sampled product",
                                 [&](ScaleScratch* sc, hipStream_t s, COut* out) { return sddmm_run<T>(sc, s, A, p, C, info, out); });
    if (rc == SPECK_OK && info) {
        info->entries = A->nnz;
        info->terms = A->nnz * p->k;
        info->lanes = lanes_of(p->k);
    }
    return rc;
}

}  // namespace

extern "C" {

int speck_sddmm_f64(speck_config* cfg, const speck_dcsr* A, const speck_sddmm_params* p, speck_dcsr* C, speck_sddmm_info* info)
{
    return sddmm_impl<double>(cfg, A, p, C, info);
}

int speck_sddmm_f32(speck_config* cfg, const speck_dcsr* A, const speck_sddmm_params* p, speck_dcsr* C, speck_sddmm_info* info)
{
    return sddmm_impl<float>(cfg, A, p, C, info);
}

int speck_sddmm_f64_b32(speck_config* cfg, const speck_dcsr* A, const speck_sddmm_params_b32* p, speck_dcsr* C, speck_sddmm_info* info)
{
    return sddmm_impl<double>(cfg, A, p, C, info);
}

int speck_sddmm_f32_b32(speck_config* cfg, const speck_dcsr* A, const speck_sddmm_params_b32* p, speck_dcsr* C, speck_sddmm_info* info)
{
    return sddmm_impl<float>(cfg, A, p, C, info);
}

}  // extern "C"
