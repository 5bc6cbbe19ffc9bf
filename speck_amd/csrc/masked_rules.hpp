// masked_rules.hpp -- the decision rules of speck_multiply_masked_* (masked.hip), each a constexpr function of integers:
// which list a row with work joins, how large a row's LDS table is and where a column lives in it, which of the two
// product walks a batch of a group kernel takes, where the per-row product count of the classifying pass saturates.
// The kernels call these; tests/cpp/masked_probe.cpp compiles the same header for the host (no HIP runtime is needed
// beyond the __host__ / __device__ words) and tests/test_masked_edges_host.py holds its answers against a literal table.
#pragma once
#include "device_common.hpp"
#include "../../include/speck_c_api.h"

namespace speck {

constexpr u32 kMaskGroupMax = SPECK_MASK_GROUP_MAX, kMaskLdsMax = SPECK_MASK_LDS_MAX;
constexpr u32 kMaskLdsSmall = 1024;  // LDS class: rows up to this many entries take the 256-thread launch
static_assert(kMaskGroupMax == 256 && kMaskLdsMax <= 4096, "group widths / 16-bit table positions");
enum { LIST_G8 = 0, LIST_G16, LIST_G32, LIST_G64, LIST_LDS_S, LIST_LDS_L, LIST_GLOBAL, MASK_LISTS };

// The products of a row as the classifying pass counts them (s_ops): it only picks a group width, so it saturates well
// below 2^32 -- nothing is added once the count has reached the ceiling, and one add brings at most the cap.
constexpr u32 kMaskOpsCeiling = 1u << 20, kMaskOpsAddCap = 1u << 20;

// The list of a row with work: `len` entries in its mask row (>= 1), `ops` products as s_ops holds them; group_max and
// lds_max are the options mask_group_max / mask_lds_max.  Group class: four mask entries per lane at most -- and not more
// than ~32 products per lane where a wider group can help.
__host__ __device__ constexpr u32 mask_list_of(u32 len, u32 ops, u32 group_max, u32 lds_max)
{
    if (len <= group_max && len <= kMaskGroupMax) {
        const u32 by_len = (len + 3u) / 4u, by_ops = ops / 32u;
        const u32 want = by_len > by_ops ? by_len : by_ops;
        return want <= 8 ? LIST_G8 : want <= 16 ? LIST_G16 : want <= 32 ? LIST_G32 : LIST_G64;
    }
    if (len <= lds_max && len <= kMaskLdsMax) return len <= kMaskLdsSmall ? LIST_LDS_S : LIST_LDS_L;
    return LIST_GLOBAL;
}

// LDS class: a row's table is the smallest power of two >= twice its length (load <= 1/2), 16 slots at least.
__host__ __device__ constexpr u32 mask_table_bits(u32 n)
{
    u32 bits = 4;
    while ((1u << bits) < 2u * n) ++bits;
    return bits;
}

// ... and the home slot of column c in a table of 2^bits slots (probing from there is linear and wraps)
__host__ __device__ constexpr u32 table_slot(u32 c, u32 bits) { return (c * 0x9E3779B1u) >> (32u - bits); }

// Group class: a batch of nb entries of A with `total` products takes the team walk where the rows of B hold 16 entries
// on average, the flattened walk otherwise.
__host__ __device__ constexpr bool mask_team_walk(u32 total, u32 nb) { return total >= 16u * nb; }

}  // namespace speck
