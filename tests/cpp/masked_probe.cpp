// masked_probe -- the decision rules of the masked product (speck_amd/csrc/masked_rules.hpp), compiled for the host and
// driven from stdin (tests/test_masked_edges_host.py).  One query per line, one answer line per query:
//   L len ops group_max lds_max  -> mask_list_of(..): 0 G8, 1 G16, 2 G32, 3 G64, 4 LDS small, 5 LDS large, 6 global
//   B n                          -> mask_table_bits(n)
//   S c bits                     -> table_slot(c, bits)
//   W total nb                   -> mask_team_walk(total, nb): 1 team walk, 0 flattened walk
//   K                            -> "kMaskOpsCeiling kMaskOpsAddCap kMaskGroupMax kMaskLdsMax kMaskLdsSmall MASK_LISTS"
#include <cstdio>

#include "masked_rules.hpp"

// the rules are usable in constant expressions on the host
static_assert(speck::mask_list_of(1, 0, 256, 4096) == speck::LIST_G8 && speck::mask_table_bits(1) == 4, "constexpr rules");

int main()
{
    using namespace speck;
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned v[4] = {};
        if (line[0] == 'L' && std::sscanf(line + 1, "%u %u %u %u", v, v + 1, v + 2, v + 3) == 4) {
            std::printf("%u\n", mask_list_of(v[0], v[1], v[2], v[3]));
        } else if (line[0] == 'B' && std::sscanf(line + 1, "%u", v) == 1) {
            std::printf("%u\n", mask_table_bits(v[0]));
        } else if (line[0] == 'S' && std::sscanf(line + 1, "%u %u", v, v + 1) == 2) {
            std::printf("%u\n", table_slot(v[0], v[1]));
        } else if (line[0] == 'W' && std::sscanf(line + 1, "%u %u", v, v + 1) == 2) {
            std::printf("%u\n", mask_team_walk(v[0], v[1]) ? 1u : 0u);
        } else if (line[0] == 'K') {
            std::printf("%u %u %u %u %u %u\n", kMaskOpsCeiling, kMaskOpsAddCap, kMaskGroupMax, kMaskLdsMax, kMaskLdsSmall,
                        (unsigned)MASK_LISTS);
        } else {
            std::printf("error: bad query\n");
        }
    }
    return 0;
}
