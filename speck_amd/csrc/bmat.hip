// bmat.hip -- speck_bmat_*: C = bmat(grid): a device CSR assembled from a grid of device CSR blocks (vstack, hstack,
// block_diag and the 2 x 2 block system are grids of one column, one row, the diagonal and four cells).  Row R0_g + i of C
// is the concatenation, in ascending block column, of row i of every block of block row g, each column id shifted by the
// origin of its block column, each value copied bit for bit.  The reference has no counterpart.
//
// The host decides the shape (bmat_plan: what speck_bmat_layout returns) and knows nnz(C) = the sum of the blocks' nnz before
// anything runs, so C's buffers are prepared first and the call reads its status block ONCE, at the end.  A PIECE is
// (output row, block present in that row's block row); the pieces in output order are the entries of C in output order.
// The block rows that hold an output row are the GROUPS of the device tables (neighbours without a block are one group).
//
//   bmat_check_kernel   a thread per piece: its group by a search in P0, its row and block by a division; the family's check
//                       of that row's two offsets (entry_tiles.hpp); the length -- 0 where they are unsound: clamped, never
//                       followed.  The shared scan (scan.hpp) over the lengths gives G.
//   bmat_tile_kernel    one workgroup per tile of 4096 output entries, four consecutive ones per thread, whatever the row and
//                       block sizes.  The UNITS of a tile: where every group it touches holds a single block (vstack,
//                       block_diag) the units are those blocks themselves -- two searches in the host-made entry origins E0,
//                       a shift per block, neither G nor a row offset is read; otherwise the pieces -- two searches in G, per
//                       piece its end, its source offset and its block in LDS (up to 4096; a tile that more units touch
//                       reads them from global memory).  First launch, kWrite = false: every id is compared with its OWN
//                       block's cols, nothing is written.  Second launch: ids shifted, values moved as integers.
//   bmat_rows_kernel    C.row_offsets[r] = G[first piece of r], staged for offset_stats_kernel and stored to C.
// Every kernel that follows G or writes into C's buffers is queued behind the check and returns at once where the verdict
// is raised.  The host side is the side operations' own (side_call.hpp: the frame of the call; compact.hpp: C).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bmat.hpp"
#include "compact.hpp"
#include "entry_tiles.hpp"
#include "launch.hpp"
#include "scan.hpp"
#include "side_call.hpp"

using namespace speck;

namespace {

constexpr u32 kTile = SPECK_BMAT_TILE_ENTRIES, kThreads = 1024, kPer = 4;
constexpr u32 kTileUnits = 4096;  // units of a tile whose ends, offsets and blocks LDS holds
constexpr u32 kCheckGrid = 2048;  // workgroups of the grid-stride kernels
constexpr u64 kDimMax = 1ull << 27;
static_assert(kTile == kThreads * kPer, "a thread holds four consecutive entries");
static_assert(SPECK_BMAT_MAX_BLOCKS <= 65536, "a block's place in the table fits 16 bits (s_blk)");

struct BmatStatus {
    u32 invalid;  // offsets of a block, an id >= its block's cols
    u32 max_row;  // the longest row of C
    unsigned long long rows_empty;
};

// a cell of the grid as the device sees it; `base` (the block's first offset) is read from ro[0] where it is needed
struct BlockDesc {
    const u32 *ro, *col;
    const void* val;
    u64 nnz;
    u32 rows, cols, c0, pad;
};

struct BmatArgs {
    const BlockDesc* blk;  // the cells by (block row, block column)
    // the groups: first output row, first piece, first entry (ng + 1 each), groups of more than one block in front (ng + 1)
    const u32 *R0, *P0, *E0, *M;
    const uint2* grp;  // (first block of the table, blocks) per group
    const u32* G;      // scan of the piece lengths: pieces + 1
    u32 ng, pieces, rows, nnz;
};

// ------------------------------------------------------------------------------------------------ the host's plan
struct Plan {
    u64 rows = 0, cols = 0, nnz = 0, pieces = 0;
    std::vector<u32> order;  // the cells by (block row, block column): the order of the device table
    std::vector<u32> c0;     // per cell of p->blocks: the origin of its block column
    std::vector<u32> R0, P0, E0, M;
    std::vector<uint2> grp;
};

// The origins of the block columns (by_col: the cells by block column); origins: block_cols + 1 entries or null.
int plan_columns(const speck_bmat_params* p, const std::vector<u32>& by_col, Plan* plan, u64* origins, bool* dim)
{
    const size_t n = p->n_blocks;
    u64 at = 0;
    size_t k = 0;
    for (u64 q = 0; q < p->block_cols; ++q) {
        const size_t k0 = k;
        while (k < n && p->blocks[by_col[k]].block_col == q) ++k;
        if (!p->col_sizes && k == k0) return SPECK_ERR_INVALID;  // a line with neither a block nor a size
        const u64 w = p->col_sizes ? p->col_sizes[q] : p->blocks[by_col[k0]].M->cols;
        for (size_t j = k0; j < k; ++j) {
            if (p->blocks[by_col[j]].M->cols != w) return SPECK_ERR_INVALID;
            plan->c0[by_col[j]] = (u32)at;
        }
        if (origins) origins[q] = at;
        if (w > kDimMax) *dim = true;
        else at += w;
        if (at > kDimMax) *dim = true;
    }
    if (origins) origins[p->block_cols] = at;
    plan->cols = at;
    return SPECK_OK;
}

// ... and of the block rows, with the groups (want_groups) the kernels walk
int plan_rows(const speck_bmat_params* p, Plan* plan, u64* origins, bool want_groups, bool* dim)
{
    const size_t n = p->n_blocks;
    const std::vector<u32>& order = plan->order;
    u64 at = 0, pieces = 0, entries = 0;
    u32 multi = 0;
    size_t k = 0;
    for (u64 g = 0; g < p->block_rows; ++g) {
        const size_t k0 = k;
        while (k < n && p->blocks[order[k]].block_row == g) ++k;
        const u64 nb = k - k0;
        if (!p->row_sizes && nb == 0) return SPECK_ERR_INVALID;
        const u64 h = p->row_sizes ? p->row_sizes[g] : p->blocks[order[k0]].M->rows;
        u64 line_nnz = 0;
        for (size_t j = k0; j < k; ++j) {
            if (p->blocks[order[j]].M->rows != h) return SPECK_ERR_INVALID;
            line_nnz += p->blocks[order[j]].M->nnz;
        }
        if (origins) origins[g] = at;
        if (h > kDimMax) *dim = true;
        if (*dim) continue;
        const bool joins = nb == 0 && !plan->grp.empty() && plan->grp.back().y == 0;  // (its extent: up to the next group's first row)
        if (want_groups && h > 0 && !joins) {
            plan->R0.push_back((u32)at), plan->P0.push_back((u32)pieces), plan->E0.push_back((u32)entries), plan->M.push_back(multi);
            plan->grp.push_back(make_uint2((u32)k0, (u32)nb));
            multi += nb > 1;
        }
        at += h, pieces += h * nb, entries += line_nnz;
        if (at > kDimMax) *dim = true;
    }
    if (origins) origins[p->block_rows] = at;
    if (want_groups) plan->R0.push_back((u32)at), plan->P0.push_back((u32)pieces), plan->E0.push_back((u32)entries), plan->M.push_back(multi);
    plan->rows = at, plan->pieces = pieces, plan->nnz = entries;
    return SPECK_OK;
}

// Everything the host decides: the arguments, the shape, the origins, nnz and the pieces.  Writes nothing but *plan and, once
// nothing can be refused any more, the caller's origin arrays.
int bmat_plan(const speck_bmat_params* p, Plan* plan, u64* row_origins, u64* col_origins, bool want_groups)
{
    if (!p) return SPECK_ERR_INVALID;
    if (p->n_blocks > SPECK_BMAT_MAX_BLOCKS) return SPECK_ERR_DIM_LIMIT;
    const size_t n = p->n_blocks;
    if (n && !p->blocks) return SPECK_ERR_INVALID;
    for (size_t b = 0; b < n; ++b) {
        const speck_bmat_block& c = p->blocks[b];
        if (!c.M || c.block_row >= p->block_rows || c.block_col >= p->block_cols) return SPECK_ERR_INVALID;
    }
    bool dim = false;
    u64 nnz = 0;
    for (size_t b = 0; b < n; ++b) {
        const speck_dcsr* M = p->blocks[b].M;
        if (M->rows > kDimMax || M->cols > kDimMax) dim = true;
        else if (M->nnz < (1ull << 32) && (!csr_args_ok(M, true) || (M->nnz && (M->rows == 0 || M->cols == 0)))) return SPECK_ERR_INVALID;
        nnz += std::min<u64>(M->nnz, 1ull << 32);  // (65536 blocks at most: the sum stays below 2^49)
    }
    // a line with neither a block nor a size (asked before a loop over lines that nothing bounds)
    if ((!p->row_sizes && p->block_rows > n) || (!p->col_sizes && p->block_cols > n)) return SPECK_ERR_INVALID;
    plan->order.resize(n), plan->c0.assign(n, 0u);
    std::vector<u32> by_col(n);
    for (size_t b = 0; b < n; ++b) plan->order[b] = by_col[b] = (u32)b;
    std::sort(plan->order.begin(), plan->order.end(), [&](u32 a, u32 b) {
        const speck_bmat_block &x = p->blocks[a], &y = p->blocks[b];
        return x.block_row != y.block_row ? x.block_row < y.block_row : x.block_col < y.block_col;
    });
    for (size_t k = 1; k < n; ++k) {
        const speck_bmat_block &x = p->blocks[plan->order[k - 1]], &y = p->blocks[plan->order[k]];
        if (x.block_row == y.block_row && x.block_col == y.block_col) return SPECK_ERR_INVALID;  // a cell named twice
    }
    std::sort(by_col.begin(), by_col.end(), [&](u32 a, u32 b) { return p->blocks[a].block_col < p->blocks[b].block_col; });
    int rc = plan_columns(p, by_col, plan, nullptr, &dim);
    if (rc != SPECK_OK) return rc;
    rc = plan_rows(p, plan, nullptr, want_groups, &dim);
    if (rc != SPECK_OK) return rc;
    if (dim) return SPECK_ERR_DIM_LIMIT;
    if (nnz >= (1ull << 32)) return SPECK_ERR_NNZ_OVERFLOW;
    if (plan->pieces >= (1ull << 32)) return SPECK_ERR_DIM_LIMIT;
    if (row_origins || col_origins) {  // (nothing is refused any more: the second walk only writes)
        Plan again;
        again.order = plan->order, again.c0.assign(n, 0u);
        if (col_origins) (void)plan_columns(p, by_col, &again, col_origins, &dim);
        if (row_origins) (void)plan_rows(p, &again, row_origins, false, &dim);
    }
    return SPECK_OK;
}

// ------------------------------------------------------------------------------------------------ pieces and units
// piece pi: its block (place in the table) and its row inside that block
__device__ __forceinline__ void piece_of(const BmatArgs& a, u32 pi, u32* blk, u32* row)
{
    const u32 g = first_end_beyond(a.P0 + 1, a.ng, pi);
    const uint2 gr = a.grp[g];
    const u32 d = pi - a.P0[g], i = d / gr.y;
    *blk = gr.x + (d - i * gr.y);
    *row = i;
}

// Unit u of a tile -- group u (kByGroup: every group of the tile holds one block or none) or piece u: the place in the table
// of its block and its source offset: output entry e of the unit lies at off + e in the block's buffers, modulo 2^32.
template <bool kByGroup>
__device__ __forceinline__ void unit_of(const BmatArgs& a, u32 u, u32* off, u32* blk)
{
    if constexpr (kByGroup) {
        const uint2 gr = a.grp[u];
        *blk = gr.x;
        *off = gr.y ? a.blk[gr.x].ro[0] - a.E0[u] : 0u;  // (a group without a block holds no entry: nobody asks)
    } else {
        u32 row;
        piece_of(a, u, blk, &row);
        *off = a.blk[*blk].ro[row] - a.G[u];
    }
}

// ------------------------------------------------------------------------------------------------ check
__global__ __launch_bounds__(256) void bmat_check_kernel(const BmatArgs a, u32* __restrict__ piece_len, BmatStatus* st)
{
    SPECK_POISON();
    bool bad = false;
    for (u64 pi = u64(blockIdx.x) * blockDim.x + threadIdx.x; pi < a.pieces; pi += u64(gridDim.x) * blockDim.x) {
        u32 blk, row;
        piece_of(a, (u32)pi, &blk, &row);
        const BlockDesc b = a.blk[blk];
        bool empty;
        const bool sound = row_offsets_sound<kTile>(b.ro, row, b.rows, b.ro[0], b.nnz, 0u, nullptr, &empty);
        piece_len[pi] = sound ? b.ro[row + 1] - b.ro[row] : 0u;
        bad |= !sound;
    }
    if (bad) st->invalid = 1;
}

// ------------------------------------------------------------------------------------------------ rows
// r <= rows: the offset of row r is G at the row's first piece (rows: G[pieces]).  Staged in new_ro for the statistics; stored
// to C where the verdict is not raised (the checks have completed: they are queued in front).
__global__ __launch_bounds__(256) void bmat_rows_kernel(const BmatArgs a, u32* __restrict__ new_ro, u32* __restrict__ c_ro,
                                                        const BmatStatus* st)
{
    SPECK_POISON();
    const bool store = st->invalid == 0;
    for (u64 r = u64(blockIdx.x) * blockDim.x + threadIdx.x; r <= a.rows; r += u64(gridDim.x) * blockDim.x) {
        u32 pi = a.pieces;
        if (r < a.rows) {
            const u32 g = first_end_beyond(a.R0 + 1, a.ng, (u32)r);
            pi = a.P0[g] + ((u32)r - a.R0[g]) * a.grp[g].y;
        }
        const u32 o = a.G[pi];
        new_ro[r] = o;
        if (store) c_ro[r] = o;
    }
}

// ------------------------------------------------------------------------------------------------ tiles
// The thread's cnt <= kPer consecutive output entries from e on: src[j] = the place of entry e + j in the buffers of block
// bk[j].  One search for the first, a walk over the ends for the others.
template <bool kByGroup, bool kLds>
__device__ __forceinline__ void thread_entries(const BmatArgs& a, const u32* s_end, const u32* s_off, const unsigned short* s_blk, u32 u0,
                                               u32 nu, u32 e, u32 cnt, u32 (&src)[kPer], u32 (&bk)[kPer])
{
    const u32* end = kLds ? s_end : (kByGroup ? a.E0 : a.G) + u0 + 1;
    u32 at = 0, off = 0, blk = 0;
    if (cnt) {
        at = first_end_beyond(end, nu, e);
        if constexpr (kLds) off = s_off[at], blk = s_blk[at];
        else unit_of<kByGroup>(a, u0 + at, &off, &blk);
    }
#pragma unroll
    for (u32 j = 0; j < kPer; ++j) {
        if (j && j < cnt && end[at] <= e + j) {
            do ++at; while (end[at] <= e + j);  // (ends below nu: the tile's last unit ends beyond its last entry)
            if constexpr (kLds) off = s_off[at], blk = s_blk[at];
            else unit_of<kByGroup>(a, u0 + at, &off, &blk);
        }
        src[j] = off + e + j;
        bk[j] = blk;
    }
}

template <typename V>
struct Vec16;
template <>
struct Vec16<u32> {
    uint4 w[1];
};
template <>
struct Vec16<u64> {
    ulonglong2 w[2];
};

__device__ __forceinline__ bool on_16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// V: the values as integers of their width (u32 / u64): bits move, nothing is computed.  kWrite = false: the ids against
// their blocks' cols, nothing is written.
template <typename V, bool kWrite>
__global__ __launch_bounds__(kThreads) void bmat_tile_kernel(const BmatArgs a, BmatStatus* st, u32* __restrict__ c_col, V* __restrict__ c_val)
{
    SPECK_POISON();
    __shared__ u32 s_end[kTileUnits], s_off[kTileUnits];
    __shared__ unsigned short s_blk[kTileUnits];
    __shared__ u32 s_head[4], s_stop;
    const u32 t = threadIdx.x;
    const u32 e0 = blockIdx.x * kTile, e1 = (u32)std::min<u64>(u64(e0) + kTile, a.nnz);
    if (t == 0) s_head[0] = first_end_beyond(a.E0 + 1, a.ng, e0);
    if (t == 64) s_head[1] = first_end_beyond(a.E0 + 1, a.ng, e1 - 1u);
    if (t == 128) s_stop = st->invalid;
    __syncthreads();
    if (s_stop) return;  // (one word for the workgroup: unsound offsets leave a G nobody may follow; a raised verdict, nothing to write)
    const u32 g0 = s_head[0], g1 = s_head[1];
    const bool by_group = a.M[g1 + 1] == a.M[g0];  // no group of several blocks among those of the tile
    u32 u0 = g0, nu = g1 - g0 + 1u;
    if (!by_group) {
        if (t == 0) s_head[2] = first_end_beyond(a.G + 1, a.pieces, e0);
        if (t == 64) s_head[3] = first_end_beyond(a.G + 1, a.pieces, e1 - 1u);
        __syncthreads();
        u0 = s_head[2], nu = s_head[3] - u0 + 1u;
    }
    const bool lds = nu <= kTileUnits;
    if (lds) {
        for (u32 k = t; k < nu; k += kThreads) {
            u32 off, blk;
            if (by_group) unit_of<true>(a, u0 + k, &off, &blk);
            else unit_of<false>(a, u0 + k, &off, &blk);
            s_end[k] = by_group ? a.E0[u0 + k + 1] : a.G[u0 + k + 1];
            s_off[k] = off;
            s_blk[k] = (unsigned short)blk;
        }
        __syncthreads();
    }
    const u32 e = e0 + t * kPer;
    const u32 cnt = e >= e1 ? 0u : e1 - e < kPer ? e1 - e : kPer;
    u32 src[kPer], bk[kPer];
    if (lds) thread_entries<false, true>(a, s_end, s_off, s_blk, u0, nu, e, cnt, src, bk);
    else if (by_group) thread_entries<true, false>(a, s_end, s_off, s_blk, u0, nu, e, cnt, src, bk);
    else thread_entries<false, false>(a, s_end, s_off, s_blk, u0, nu, e, cnt, src, bk);
    if (!cnt) return;
    const bool one_block = cnt == kPer && bk[0] == bk[1] && bk[1] == bk[2] && bk[2] == bk[3];
    u32 id[kPer];
    V v[kPer];
    if (one_block) {
        const BlockDesc b = a.blk[bk[0]];
        // one piece, or pieces of rows that follow each other in the buffers (the rows of one block ascend with the entries)
        const bool run = src[kPer - 1] - src[0] == kPer - 1u;
        if (run && on_16(b.col + src[0])) {
            const uint4 q = *reinterpret_cast<const uint4*>(b.col + src[0]);
            id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
        } else {
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) id[j] = b.col[src[j]];
        }
        if constexpr (kWrite) {
            const V* val = static_cast<const V*>(b.val);
            if (run && on_16(val + src[0])) {
                const Vec16<V> q = *reinterpret_cast<const Vec16<V>*>(val + src[0]);
                __builtin_memcpy(v, &q, sizeof q);
            } else {
#pragma unroll
                for (u32 j = 0; j < kPer; ++j) v[j] = val[src[j]];
            }
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) id[j] += b.c0;
        } else {
            bool bad = false;
#pragma unroll
            for (u32 j = 0; j < kPer; ++j) bad |= id[j] >= b.cols;
            if (bad) st->invalid = 1;
        }
    } else {
        bool bad = false;
#pragma unroll
        for (u32 j = 0; j < kPer; ++j) {
            if (j >= cnt) continue;
            const BlockDesc* b = a.blk + bk[j];
            id[j] = b->col[src[j]];
            if constexpr (kWrite) {
                v[j] = static_cast<const V*>(b->val)[src[j]];
                id[j] += b->c0;
            } else bad |= id[j] >= b->cols;
        }
        if (!kWrite && bad) st->invalid = 1;
    }
    if constexpr (kWrite) {
        // entry e + j goes to place e + j: four ids are 16 bytes at a multiple of 16 from the buffer's start
        if (cnt == kPer && on_16(c_col + e) && on_16(c_val + e)) {
            *reinterpret_cast<uint4*>(c_col + e) = make_uint4(id[0], id[1], id[2], id[3]);
            Vec16<V> q;
            __builtin_memcpy(&q, v, sizeof q);
            *reinterpret_cast<Vec16<V>*>(c_val + e) = q;
        } else {
#pragma unroll
            for (u32 j = 0; j < kPer; ++j)
                if (j < cnt) c_col[e + j] = id[j], c_val[e + j] = v[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
// the tables of a call as one block of bytes: what the kernels read beside the blocks themselves
struct Tables {
    std::vector<unsigned char> bytes;
    size_t at_R0, at_P0, at_E0, at_M, at_grp;
};

void build_tables(const speck_bmat_params* p, const Plan& plan, Tables* t)
{
    const size_t n = plan.order.size(), ng = plan.grp.size();
    const size_t blk_bytes = up256(std::max<size_t>(n, 1) * sizeof(BlockDesc)), line = up256((ng + 1) * 4), grp_bytes = up256(std::max<size_t>(ng, 1) * sizeof(uint2));
    t->at_R0 = blk_bytes, t->at_P0 = blk_bytes + line, t->at_E0 = blk_bytes + 2 * line, t->at_M = blk_bytes + 3 * line, t->at_grp = blk_bytes + 4 * line;
    t->bytes.assign(t->at_grp + grp_bytes, 0);
    BlockDesc* d = reinterpret_cast<BlockDesc*>(t->bytes.data());
    for (size_t k = 0; k < n; ++k) {
        const speck_dcsr* M = p->blocks[plan.order[k]].M;
        d[k] = BlockDesc{M->row_offsets, M->col_ids, M->data, M->nnz, (u32)M->rows, (u32)M->cols, plan.c0[plan.order[k]], 0u};
    }
    std::memcpy(t->bytes.data() + t->at_R0, plan.R0.data(), (ng + 1) * 4);
    std::memcpy(t->bytes.data() + t->at_P0, plan.P0.data(), (ng + 1) * 4);
    std::memcpy(t->bytes.data() + t->at_E0, plan.E0.data(), (ng + 1) * 4);
    std::memcpy(t->bytes.data() + t->at_M, plan.M.data(), (ng + 1) * 4);
    if (ng) std::memcpy(t->bytes.data() + t->at_grp, plan.grp.data(), ng * sizeof(uint2));
}

void fill_info(speck_bmat_info* info, const Plan& plan, u64 blocks, const BmatStatus& h)
{
    if (!info) return;
    info->blocks = blocks, info->rows_out = plan.rows, info->cols_out = plan.cols, info->nnz_out = plan.nnz, info->pieces = plan.pieces;
    info->rows_empty = h.rows_empty, info->max_row_entries = h.max_row;
}

template <typename V>
int bmat_run(BmatScratch* sc, hipStream_t s, const speck_bmat_params* p, const Plan& plan, const Tables& tab, speck_dcsr* C,
             speck_bmat_info* info, COut* out)
{
    const u32 rows = (u32)plan.rows, pieces = (u32)plan.pieces, nnz = (u32)plan.nnz, ng = (u32)plan.grp.size();
    if (rows == 0) {  // every block is without a row, so without an entry: nothing to check
        const int rc = publish_empty_c(C, plan.cols, sizeof(V), s, out);
        if (rc == SPECK_OK) fill_info(info, plan, p->n_blocks, BmatStatus{});
        return rc;
    }
    // status | tables | staged row offsets | workgroup sums of the scan
    const size_t tab_bytes = tab.bytes.size(), row_bytes = up256((size_t(rows) + 1) * 4);
    const size_t sum_bytes = up256((size_t(pieces) / 1024 + 2) * 4);
    int rc = sc->fixed.ensure(256 + tab_bytes + row_bytes + sum_bytes);
    if (rc != SPECK_OK) return rc;
    const size_t piece_bytes = up256(size_t(std::max(pieces, 1u)) * 4);
    rc = sc->var.ensure(piece_bytes + up256((size_t(pieces) + 1) * 4));
    if (rc != SPECK_OK) return rc == SPECK_ERR_OOM ? SPECK_ERR_DIM_LIMIT : rc;  // more pieces than the scratch can hold
    unsigned char* fb = static_cast<unsigned char*>(sc->fixed.p);
    static_assert(sizeof(BmatStatus) <= 256, "status block");
    BmatStatus* st = reinterpret_cast<BmatStatus*>(fb);
    unsigned char* dt = fb + 256;
    u32* new_ro = reinterpret_cast<u32*>(fb + 256 + tab_bytes);
    u32* block_sums = reinterpret_cast<u32*>(fb + 256 + tab_bytes + row_bytes);
    u32* piece_len = static_cast<u32*>(sc->var.p);
    u32* G = reinterpret_cast<u32*>(static_cast<unsigned char*>(sc->var.p) + piece_bytes);

    rc = prepare_c(C, rows, nnz, sizeof(V), out);  // (allocations only: nothing of C changes before publish_c)
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(BmatStatus), s));
    HIP_TRY(hipMemcpyAsync(dt, tab.bytes.data(), tab_bytes, hipMemcpyHostToDevice, s));  // (tab outlives the final synchronise)
    const BmatArgs a{reinterpret_cast<const BlockDesc*>(dt), reinterpret_cast<const u32*>(dt + tab.at_R0), reinterpret_cast<const u32*>(dt + tab.at_P0),
                     reinterpret_cast<const u32*>(dt + tab.at_E0), reinterpret_cast<const u32*>(dt + tab.at_M),
                     reinterpret_cast<const uint2*>(dt + tab.at_grp), G, ng, pieces, rows, nnz};

    // ---- the offsets of every row of every block, the piece lengths and their scan
    if (pieces) {
        SPECK_LAUNCH(bmat_check_kernel, dim3(grid_of((u64(pieces) + 255) / 256, kCheckGrid)), dim3(256), 0, s, a, piece_len, st);
        launch_exclusive_scan(s, CountArray{piece_len}, pieces, block_sums, G, nullptr);
    } else HIP_TRY(hipMemsetAsync(G, 0, 4, s));
    // ---- every id against its own block's cols: the tile kernel, writing nothing
    const u32 tiles = (nnz + kTile - 1) / kTile;
    if (nnz) SPECK_LAUNCH((bmat_tile_kernel<V, false>), dim3(tiles), dim3(kThreads), 0, s, a, st, static_cast<u32*>(nullptr), static_cast<V*>(nullptr));
    // ---- behind the verdict: the row offsets, their statistics, the entries
    const u32 row_grid = grid_of((u64(rows) + 256) / 256, kCheckGrid);
    SPECK_LAUNCH(bmat_rows_kernel, dim3(row_grid), dim3(256), 0, s, a, new_ro, out->ro, st);
    SPECK_LAUNCH(offset_stats_kernel, dim3(row_grid), dim3(256), 0, s, new_ro, rows, &st->max_row, &st->rows_empty);
    if (nnz) SPECK_LAUNCH((bmat_tile_kernel<V, true>), dim3(tiles), dim3(kThreads), 0, s, a, st, out->col, static_cast<V*>(out->val));
    // ---- the one read-back
    BmatStatus h{};
    rc = read_status(s, st, &h);
    if (rc != SPECK_OK) return rc;
    if (h.invalid) return SPECK_ERR_INVALID;
    publish_c(C, rows, plan.cols, nnz, out);
    fill_info(info, plan, p->n_blocks, h);
    return SPECK_OK;
}

const char* const kGuardNames[5] = {"bmat tables and row offsets", "bmat piece lengths and offsets", "C.data", "C.col_ids", "C.row_offsets"};

template <typename V>
int bmat_impl(speck_config* cfg, const speck_bmat_params* p, speck_dcsr* C, speck_bmat_info* info)
{
    if (!p || !C) return SPECK_ERR_INVALID;
    Plan plan;
    const int rc = bmat_plan(p, &plan, nullptr, nullptr, true);
    if (rc != SPECK_OK) return rc;
    for (u32 b = 0; b < p->n_blocks; ++b)
        if (shares_buffer(C, p->blocks[b].M)) return SPECK_ERR_INVALID;
    if (info) *info = speck_bmat_info{};
    if (!cfg && !device_present()) return SPECK_ERR_NO_DEVICE;
    Tables tab;  // (here, not in the body: the frame below synchronises before it returns, whatever the body did)
    build_tables(p, plan, &tab);
    return run_side_call(cfg, bmat_scratch, C, info, kGuardNames, " by the assembly",
                         [&](BmatScratch* sc, hipStream_t s, COut* out) { return bmat_run<V>(sc, s, p, plan, tab, C, info, out); });
}

}  // namespace

extern "C" {

int speck_bmat_layout(const speck_bmat_params* p, speck_bmat_layout_out* out)
{
    if (!p || !out) return SPECK_ERR_INVALID;
    Plan plan;
    const int rc = bmat_plan(p, &plan, out->row_origins, out->col_origins, false);
    if (rc != SPECK_OK) return rc;
    out->rows = plan.rows, out->cols = plan.cols, out->nnz = plan.nnz, out->pieces = plan.pieces;
    return SPECK_OK;
}

int speck_bmat_f64(speck_config* cfg, const speck_bmat_params* p, speck_dcsr* C, speck_bmat_info* info) { return bmat_impl<u64>(cfg, p, C, info); }

int speck_bmat_f32(speck_config* cfg, const speck_bmat_params* p, speck_dcsr* C, speck_bmat_info* info) { return bmat_impl<u32>(cfg, p, C, info); }

}  // extern "C"
