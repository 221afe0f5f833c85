// Host predicate of the march kernel's scaled-ray instantiation (march_span<..., SCALED = true>, DESIGN.md "Scaled ray"):
// a per-axis factor ss = size * scale qualifies when it is an exact power of two 2^m with 0 <= m <= 23.  m >= 0 makes
// start * ss and step * ss exact for every float (scaling up never rounds, subnormals included); 2^23 bounds the
// products far away from overflow.  Plain C++ (no HIP): tests/test_pow2_predicate.py compiles it on its own.
#pragma once
#include <math.h>

static inline bool svr_ss_pow2(float ss) {
    int e = 0;
    const float m = frexpf(ss, &e);                 // ss = m * 2^e, m in [0.5, 1) for finite ss > 0
    return m == 0.5f && ss >= 1.0f && ss <= 8388608.0f;
}
