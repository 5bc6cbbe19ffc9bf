// radix_pairs.hpp -- the ONE radix sort of the tree, as its callers see it: the stable least-significant-digit sort of
// (key, payload) pairs that extras.hip holds (kernels, constants and the description of a pass are there, where the
// transpose and the plan use it with column keys).  coo.hip sorts (row key, position) with it on the call's stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "device_common.hpp"

namespace speck {

// words of `hist`: one count per (digit, workgroup) -- 256 x kRadixBlocks (extras.hip asserts it)
constexpr size_t kRadixHistWords = size_t(256) * 1024;

// sorts (keys, vals) by the low `bits` bits of the keys, 8 bits per pass, on stream `s`; a/b are ping-pong buffers of n
// words each (the input is in a, the result in the returned index: 0 = a, 1 = b).  Stable.  Nothing is waited for.
int radix_sort_pairs(u32* keys_a, u32* vals_a, u32* keys_b, u32* vals_b, u32 n, unsigned bits, u32* hist, hipStream_t s);

}  // namespace speck
