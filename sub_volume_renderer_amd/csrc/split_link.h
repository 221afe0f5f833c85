// The two integer rules of svr_split (include/svr.h; kernels: split_kernels.hip) that decide its result: the order in
// which voxels beat one another, and the test by which two basins link.  Plain C++ on plain integers: the kernels and a
// host test (tests/test_split.py) compile the same text.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define SPLIT_FN __host__ __device__ __forceinline__
#else
#define SPLIT_FN inline
#endif

// The order as one unsigned key, for inside voxels (height > 0) with an index below 2^32 - 1: i beats j iff
// split_key(height[i], i) > split_key(height[j], j).  The packing svr_distance uses for its deepest point: a 64-bit
// maximum picks the greater height and, among equals, the smaller index.
SPLIT_FN uint64_t split_key(int32_t height, uint32_t index) {
    return ((uint64_t)(uint32_t)height << 32) | (uint64_t)(0xFFFFFFFFu - index);
}
SPLIT_FN uint32_t split_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
SPLIT_FN int32_t split_key_height(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }

// Do two basins link over a pass of height s > 0 when the lower of their peaks is a >= s and H = merge_squared <= 2^29?
// sqrt(a) - sqrt(s) <= sqrt(H), exactly: with t = a - s - H it reads t <= 2 sqrt(H s), which holds for t <= 0 and else
// iff t^2 <= 4 H s.  t < 2^31 and 4 H s < 2^62: both sides fit int64.
SPLIT_FN bool split_links(int32_t a, int32_t s, uint32_t H) {
    const int64_t t = (int64_t)a - (int64_t)s - (int64_t)H;
    if (t <= 0) return true;
    return t * t <= 4 * (int64_t)H * (int64_t)s;
}
