// The host-side rule of a segment table (loans_amd/csrc/seg_table.h) as a plain C++ program (see test_segtable_cpu.py): reads cases
// on stdin -- `n unit nseg count e0 .. e(count-1)`, count = -1 for a null table -- and prints seg_table_units' answer, one per line.
#include <inttypes.h>
#include <stdio.h>
#include <vector>
#include "seg_table.h"

int main() {
    int64_t n, unit;
    int nseg, count;
    while (scanf("%" SCNd64 " %" SCNd64 " %d %d", &n, &unit, &nseg, &count) == 4) {
        std::vector<int64_t> ends(count > 0 ? count : 0);
        for (int64_t& e : ends)
            if (scanf("%" SCNd64, &e) != 1) return 2;
        printf("%" PRId64 "\n", seg_table_units(count < 0 ? nullptr : ends.data(), nseg, n, unit));
    }
    printf("limit %d\n", SEG_MAX_SEGMENTS);
    return 0;
}
