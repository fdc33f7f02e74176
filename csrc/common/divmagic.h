// Exact u32 division by a launch-time constant, for the flat K3 fan-out's
// unit -> (pair, unit-in-pair) index math (csrc/hip/dataplane.hip).  Plain
// host C++ so csrc/tests/test_native.cpp can check the exactness claim.
#pragma once

#include <stdint.h>

// exact u32 division-by-constant: p = (f * m) >> sh for all f < 2^31,
// 1 <= d <= 2^21 (Granlund-Montgomery with one headroom bit: l = ceil_log2 d,
// m = ceil(2^(31+l)/d) < 2^32, sh = 31+l; m*d - 2^(31+l) < d <= 2^l)
static inline void u32_div_magic(int32_t d, uint32_t* m, int32_t* sh) {
    int l = 0;
    while ((1u << l) < (uint32_t)d) ++l;  // ceil_log2(d), d >= 1
    *m = (uint32_t)(((1ull << (31 + l)) + (uint64_t)d - 1) / (uint64_t)d);
    *sh = 31 + l;
}
