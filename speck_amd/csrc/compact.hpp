// compact.hpp -- what the operations that keep a SUBSET of a matrix's entries share (the masked product: the mask entries
// with a hit; the filter: the entries of A its predicates keep): the keep bytes read a word of four at a time, the
// streaming compaction behind the shared scan (scan.hpp) over those words, and the rule by which C takes its buffers.
//   KeepWord                 functor for launch_exclusive_scan: the kept entries among entries 4 i .. 4 i + 3
//   compact_entries_kernel   4096 entries per workgroup: an entry's place is the number of kept entries in front of it --
//                            its workgroup's scanned sum + its place inside the workgroup; (column, value) copied there.
//                            The values come from an array of S and go to one of T (the masked product's accumulators are
//                            double whatever T is; the filter copies T to T, bit for bit)
//   COut / prepare_c / publish_c   C's buffers by the multiply's rule; nothing of C changes before publish_c
//   publish_empty_c / finish_rows / finish_subset   how a call ends: no rows; offsets copied, C published; compaction first
//   csr_args_ok / shares_buffer    the argument checks both entry points make before anything touches a device
#pragma once
#include <algorithm>

#include "host_common.hpp"
#include "launch.hpp"
#include "scan.hpp"

namespace speck {

// The compaction needs no rows: the kept entries stay in their order, so an entry's place is the number of kept entries in
// front of it -- the shared scan over the keep bytes, a word of four per item (4096 entries per workgroup), as far as the
// scanned workgroup sums; the kernel below places the four entries of a thread itself.  (First form, masked product:
// eight lanes per row looking up the row's new offset -- 0.37 ms for the 1 M short rows of the webbase stand-in.)
constexpr u32 kCompactTile = 4096;

struct KeepWord {
    const u32* keep32;  // one byte per entry, bit 0: kept
    u64 n;              // entries
    // the keep bytes of entries 4 i .. 4 i + 3, a bit each
    __device__ __forceinline__ u32 word(u32 i) const
    {
        const u64 e0 = u64(i) * 4;
        if (e0 >= n) return 0u;
        u32 w = keep32[i] & 0x01010101u;
        if (e0 + 4 > n) w &= 0xFFFFFFFFu >> (8u * (u32)(e0 + 4 - n));  // (the bytes behind the last entry were never written)
        return w;
    }
    __device__ __forceinline__ u32 operator()(u32 i) const { return (u32)__popc(word(i)); }
};

#ifdef __HIPCC__
template <typename S, typename T>
static __global__ __launch_bounds__(1024) void compact_entries_kernel(const KeepWord f, const u32* __restrict__ tile_sums,
                                                                      const u32* __restrict__ src_col,
                                                                      const S* __restrict__ src_val, u32* __restrict__ c_col,
                                                                      T* __restrict__ c_val)
{
    SPECK_POISON();
    __shared__ u32 s_scan[1024 / 64 + 1];
    const u32 i = blockIdx.x * 1024u + threadIdx.x;
    const u64 e0 = u64(i) * 4;
    const u32 w = f.word(i);
    u32 total;
    u32 to = tile_sums[blockIdx.x] + block_exclusive_scan<1024>((u32)__popc(w), s_scan, &total);
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        if ((w >> (8u * k)) & 1u) {
            c_col[to] = src_col[e0 + k];
            c_val[to] = (T)src_val[e0 + k];
            ++to;
        }
}
#endif

// The buffers C will own once the call has completed, by the multiply's rule: row_offsets reused when C->rows == rows(A),
// data / col_ids re-allocated only when C->nnz differs.  Nothing of C changes before publish_c().
struct COut {
    u32* ro = nullptr;
    u32* col = nullptr;
    void* val = nullptr;
    bool own_ro = false, own_data = false;
    void discard()
    {
        if (own_ro && ro) (void)guarded_free(ro);
        if (own_data && col) (void)guarded_free(col);
        if (own_data && val) (void)guarded_free(val);
        *this = COut{};
    }
};

inline int prepare_c(const speck_dcsr* C, u64 rows, u64 nnz_out, size_t vsize, COut* out)
{
    if (C->rows == rows && C->row_offsets) out->ro = C->row_offsets;
    else {
        HIP_TRY(guarded_malloc(reinterpret_cast<void**>(&out->ro), (size_t(rows) + 1) * sizeof(u32)));
        out->own_ro = true;
    }
    if (C->nnz != nnz_out || !C->data || !C->col_ids) {
        out->own_data = true;
        const hipError_t e1 = guarded_malloc(&out->val, std::max<size_t>(nnz_out, 1) * vsize);
        const hipError_t e2 = e1 == hipSuccess ? guarded_malloc(reinterpret_cast<void**>(&out->col), std::max<size_t>(nnz_out, 1) * 4) : e1;
        if (e1 != hipSuccess || e2 != hipSuccess) {
            (void)hipGetLastError();
            out->discard();
            return SPECK_ERR_OOM;
        }
    } else {
        out->val = C->data;
        out->col = C->col_ids;
    }
    return SPECK_OK;
}

inline void publish_c(speck_dcsr* C, u64 rows, u64 cols, u64 nnz_out, COut* out)
{
    if (out->own_data) {
        if (C->data) (void)guarded_free(C->data);
        if (C->col_ids) (void)guarded_free(C->col_ids);
    }
    if (C->row_offsets && C->row_offsets != out->ro) (void)guarded_free(C->row_offsets);
    C->rows = rows, C->cols = cols, C->nnz = nnz_out;
    C->data = out->val, C->col_ids = out->col, C->row_offsets = out->ro;
    *out = COut{};
}

// a result without rows: one offset, 0
inline int publish_empty_c(speck_dcsr* C, u64 cols, size_t vsize, hipStream_t s, COut* out)
{
    const int rc = prepare_c(C, 0, 0, vsize, out);
    if (rc != SPECK_OK) return rc;
    HIP_TRY(hipMemsetAsync(out->ro, 0, sizeof(u32), s));
    HIP_TRY(hipStreamSynchronize(s));
    publish_c(C, 0, cols, 0, out);
    return SPECK_OK;
}

// the end of a call whose kernels (queued on `s`) fill `out`: the new row offsets copied over, the stream drained, C published
inline int finish_rows(hipStream_t s, const u32* new_ro, u32 rows, u64 cols, u64 nnz_out, speck_dcsr* C, COut* out)
{
    HIP_TRY(hipMemcpyAsync(out->ro, new_ro, (size_t(rows) + 1) * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (take_launch_error()) return SPECK_ERR_HIP;
    publish_c(C, rows, cols, nnz_out, out);
    return SPECK_OK;
}

#ifdef __HIPCC__
// ... that keeps a subset: the nnz_out entries of (src_col, src_val) whose keep byte is set compacted into `out` first
template <typename S, typename T>
int finish_subset(hipStream_t s, const KeepWord& words, u32* tile_sums, const u32* src_col, const S* src_val, const u32* new_ro,
                  u32 rows, u64 cols, u64 nnz_out, speck_dcsr* C, COut* out)
{
    if (nnz_out) {
        launch_exclusive_scan(s, words, (u32)((words.n + 3) / 4), tile_sums, nullptr, nullptr);
        SPECK_LAUNCH((compact_entries_kernel<S, T>), dim3((u32)((words.n + kCompactTile - 1) / kCompactTile)), dim3(1024), 0, s, words,
                     tile_sums, src_col, src_val, out->col, static_cast<T*>(out->val));
    }
    return finish_rows(s, new_ro, rows, cols, nnz_out, C, out);
}
#endif

inline bool csr_args_ok(const speck_dcsr* X, bool needs_values)
{
    if (X->rows && !X->row_offsets) return false;
    if (X->nnz && (!X->col_ids || (needs_values && !X->data))) return false;
    return true;
}

inline bool shares_buffer(const speck_dcsr* C, const speck_dcsr* X)
{
    const void* mine[] = {C->data, C->col_ids, C->row_offsets};
    const void* theirs[] = {X->data, X->col_ids, X->row_offsets};
    for (const void* p : mine)
        for (const void* q : theirs)
            if (p && p == q) return true;
    return false;
}

}  // namespace speck
