// What the streaming passes over a box of one LOD's window share (object_kernels.hip; histogram_kernels.hip keeps its
// own, older copies of the same lines so that its code objects stay as they were): the cut of box and window at the
// ring's wrap seams, the u32 keys that order like floats, and the search of a sorted id list.
#pragma once

#include "svr_internal.h"

// u32 keys that order like the floats they come from (never given a NaN)
__device__ __forceinline__ uint32_t ring_key_of_float(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ring_float_of_key(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// lower-bound search; every probe lies in [0, n) whatever the order of `s`
__device__ __forceinline__ bool ring_in_set(const uint32_t* __restrict__ s, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && s[lo] == v;
}

// The box lo[a] .. lo[a] + n[a] (logical voxels of the LOD, inside its window, n > 0) cut at the ring's wrap seams:
// per axis the run up to the ring's end, then the run that wrapped to its start.  s: first ring slot, m: extent,
// cnt: 1 or 2 runs.  Returns the number of voxels.
inline size_t ring_cut_at_seams(const LodStorage& L, const int64_t lo[3], const int64_t n[3], uint32_t s[3][2], uint32_t m[3][2],
                                int cnt[3]) {
    size_t total = 1;
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t R = (uint32_t)L.ring[ax];
        int64_t s64 = lo[ax] % (int64_t)R;
        if (s64 < 0) s64 += R;
        const uint32_t s0 = (uint32_t)s64, len = (uint32_t)n[ax];     // len <= the window <= R
        const uint32_t first = len < R - s0 ? len : R - s0;
        s[ax][0] = s0; m[ax][0] = first; cnt[ax] = 1;
        if (first < len) { s[ax][1] = 0u; m[ax][1] = len - first; cnt[ax] = 2; }
        total *= (size_t)len;
    }
    return total;
}
