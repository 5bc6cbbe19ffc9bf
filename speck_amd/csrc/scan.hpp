// scan.hpp -- device-wide exclusive scan of one count per item, for the side operations (the row sort's new row lengths,
// the masked product's hits per row and per word of hit bytes).  Three launches on one stream:
//   scan_block_sums_kernel<F>   1024 items per workgroup: their sum
//   scan_sums_kernel            one workgroup: the sums scanned in place, 1024 at a time with a carry
//   scan_offsets_kernel<F>      1024 items per workgroup again: offset of item i = its workgroup's scanned sum + its place
//                               inside the workgroup; offsets_out[n] = the total
// F is a small functor passed by value: f(i) = the count of item i, i < n (never called beyond).  The counts are computed
// twice rather than stored: they are a load or two each.  The sums are 32-bit -- the callers' totals are entries of a
// matrix (< 2^32).  (The multiply's own scan, stages.hip, is another shape: one chained pass that also classifies.)
// Beside them offset_stats_kernel: the rows without an entry and the longest row of offsets a call has made.
#pragma once
#include "device_common.hpp"
#include "launch.hpp"

namespace speck {

template <typename F>
static __global__ __launch_bounds__(1024) void scan_block_sums_kernel(const F f, u32 n, u32* __restrict__ block_sums)
{
    SPECK_POISON();
    __shared__ u32 s_scan[1024 / 64 + 1];
    const u32 i = blockIdx.x * 1024u + threadIdx.x;
    u32 total;
    (void)block_exclusive_scan<1024>(i < n ? f(i) : 0u, s_scan, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

static __global__ __launch_bounds__(1024) void scan_sums_kernel(u32* __restrict__ block_sums, u32 n)
{
    SPECK_POISON();
    __shared__ u32 s_scan[1024 / 64 + 1];
    u32 carry = 0;
    for (u32 i0 = 0; i0 < n; i0 += 1024) {
        const u32 i = i0 + threadIdx.x;
        const u32 v = i < n ? block_sums[i] : 0u;
        u32 total;
        const u32 ex = block_exclusive_scan<1024>(v, s_scan, &total);
        if (i < n) block_sums[i] = carry + ex;
        carry += total;
    }
}

template <typename F>
static __global__ __launch_bounds__(1024) void scan_offsets_kernel(const F f, u32 n, const u32* __restrict__ block_sums,
                                                                   u32* __restrict__ offsets_out,
                                                                   unsigned long long* __restrict__ total_out)
{
    SPECK_POISON();
    __shared__ u32 s_scan[1024 / 64 + 1];
    const u32 i = blockIdx.x * 1024u + threadIdx.x;
    const u32 len = i < n ? f(i) : 0u;
    u32 total;
    const u32 ex = block_exclusive_scan<1024>(len, s_scan, &total);
    const u32 off = block_sums[blockIdx.x] + ex;
    if (i < n) offsets_out[i] = off;
    if (i + 1 == n) {
        offsets_out[n] = off + len;
        if (total_out) *total_out = off + len;
    }
}

// the plainest F: the counts lie in an array (the filter's kept entries per row, the addition's entries of C per row)
struct CountArray {
    const u32* count;
    __device__ u32 operator()(u32 i) const { return count[i]; }
};

// What a call reports about the rows behind such a scan (the conversion from COO, the extraction): the rows without an
// entry and the longest row of the offsets ro[0 .. rows], a wave reduction and one integer atomic per wave and counter.
static __global__ void offset_stats_kernel(const u32* __restrict__ ro, u32 rows, u32* __restrict__ longest_out,
                                           unsigned long long* __restrict__ empty_out)
{
    SPECK_POISON();
    u32 empty = 0, longest = 0;
    for (u64 r = u64(blockIdx.x) * blockDim.x + threadIdx.x; r < rows; r += u64(gridDim.x) * blockDim.x) {
        const u32 len = ro[r + 1] - ro[r];
        empty += len == 0;
        longest = max(longest, len);
    }
    empty = wave_reduce_add(empty);
    longest = wave_reduce_max(longest);
    if (lane_id() == 0) {
        if (empty) atomicAdd(empty_out, (unsigned long long)empty);
        if (longest) atomicMax(longest_out, longest);
    }
}

// n >= 1 items; block_sums: (n + 1023) / 1024 words, left holding the scanned workgroup sums.  offsets_out: n + 1 words,
// or nullptr -- the caller places the items itself, from the scanned sums (then total_out is not written either).
template <typename F>
void launch_exclusive_scan(hipStream_t s, const F& f, u32 n, u32* block_sums, u32* offsets_out, unsigned long long* total_out)
{
    const u32 nblk = (n + 1023) / 1024;
    SPECK_LAUNCH(scan_block_sums_kernel<F>, dim3(nblk), dim3(1024), 0, s, f, n, block_sums);
    SPECK_LAUNCH(scan_sums_kernel, dim3(1), dim3(1024), 0, s, block_sums, nblk);
    if (offsets_out) SPECK_LAUNCH(scan_offsets_kernel<F>, dim3(nblk), dim3(1024), 0, s, f, n, block_sums, offsets_out, total_out);
}

}  // namespace speck
