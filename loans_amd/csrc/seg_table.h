// Host-side rule of a segment table of the flat parameter arena (not part of the C ABI), stated once for momentum SGD with
// per-segment decay, LARS and LAMB.  Plain C++ as well as HIP, no HIP calls or types.  tests/arena_kernels/test_segtable_cpu.py
// owns this rule.
#pragma once
#include <stdint.h>
#include "loans_hip.h"

constexpr int SEG_MAX_SEGMENTS = LOANS_LARS_MAX_SEGMENTS;       // the kernels keep the table in LDS: 8 KB of ends, 1 KB of flags

// `ends` (host memory): exclusive, ascending, no empty segment, every end but the last a multiple of 4 -- no float4 straddles a
// boundary --, the last one at n (n < 0: any).  The number of units of `unit` floats, each segment cut on its own, or -1.
// (len - 1) / unit + 1 and not (len + unit - 1) / unit: an end near INT64_MAX must not overflow.
inline int64_t seg_table_units(const int64_t* ends, int32_t nseg, int64_t n, int64_t unit) {
    if (!ends || nseg <= 0 || nseg > SEG_MAX_SEGMENTS) return -1;
    int64_t prev = 0, units = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t e = ends[s];
        if (e <= prev || (s < nseg - 1 && (e & 3))) return -1;
        units += (e - prev - 1) / unit + 1;
        prev = e;
    }
    if (n >= 0 && prev != n) return -1;
    return units;
}
