// classify_probe -- the row classifiers and table-size rules of speck_amd/csrc/device_common.hpp, compiled for the host
// and driven from stdin (tests/test_edges_host.py).  One query per line, one answer line per query:
//   C len_a ops nnz cmin cmax  sym_bitmap_ratio num_dense_ratio num_global_passes num_w256 esc16 esc32 esc64 esc_fused
//     num_g8 sym_g8 sym_w128 nf_min_ops gh_per_window slice_ops        -> "<classify_symbolic> <classify_numeric>"
//   T nnz pct        -> table_bits(nnz, pct)
//   M cap pct        -> max_nnz_of(cap, pct)
//   G ops            -> gh_table_slots(ops)
//   S cmin cmax ops  -> nf_slot_entries(cmin, cmax, ops)
//   K                -> the load percentages the header was compiled with: "SPECK_LOAD_PCT SPECK_LOAD_TINY_PCT"
#include <cstdio>
#include <cstring>

#include "device_common.hpp"

int main()
{
    using namespace speck;
    char line[512];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned v[19] = {};
        if (line[0] == 'C') {
            const int n = std::sscanf(line + 1, "%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", v, v + 1, v + 2, v + 3,
                                      v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12, v + 13, v + 14, v + 15,
                                      v + 16, v + 17, v + 18);
            if (n != 19) {
                std::printf("error: %d of 19 fields\n", n);
                continue;
            }
            ClassifyParams p;
            std::memset(&p, 0, sizeof p);
            p.sym_bitmap_ratio = v[5], p.num_dense_ratio = v[6], p.num_global_passes = v[7], p.num_w256 = v[8];
            p.esc16 = v[9], p.esc32 = v[10], p.esc64 = v[11], p.esc_fused = v[12], p.num_g8 = v[13], p.sym_g8 = v[14];
            p.sym_w128 = v[15], p.nf_min_ops = v[16], p.gh_per_window = v[17], p.slice_ops = v[18];
            std::printf("%u %u\n", (unsigned)classify_symbolic(v[0], v[1], v[3], v[4], p),
                        (unsigned)classify_numeric(v[0], v[1], v[2], v[3], v[4], p));
        } else if (line[0] == 'T' && std::sscanf(line + 1, "%u %u", v, v + 1) == 2) {
            std::printf("%u\n", table_bits(v[0], v[1]));
        } else if (line[0] == 'M' && std::sscanf(line + 1, "%u %u", v, v + 1) == 2) {
            std::printf("%u\n", max_nnz_of(v[0], v[1]));
        } else if (line[0] == 'G' && std::sscanf(line + 1, "%u", v) == 1) {
            std::printf("%u\n", gh_table_slots(v[0]));
        } else if (line[0] == 'S' && std::sscanf(line + 1, "%u %u %u", v, v + 1, v + 2) == 3) {
            std::printf("%u\n", nf_slot_entries(v[0], v[1], v[2]));
        } else if (line[0] == 'K') {
            std::printf("%u %u\n", (unsigned)SPECK_LOAD_PCT, (unsigned)SPECK_LOAD_TINY_PCT);
        } else {
            std::printf("error: bad query\n");
        }
    }
    return 0;
}
