// The linear sample of include/svr.h ("the linear sample"), shared by slice_kernels.hip, composite_kernels.hip and
// iso_kernels.hip: the cell of a point inside the LOD that holds it (two clamped, wrapped ring slots and one fraction
// per axis), the 64-bit element offsets of its eight corners in the rows or in the micro-block copy, and the blend.
//
// Arithmetic contract: strict IEEE f32 without contraction (-ffp-contract=off), one operation per step, in the order
// svr.h states; tests/linear_twin.py restates it in numpy and the GPU suites compare values bit for bit.
//
// A sample's LOD differs from lane to lane, so the kernels first copy the few fields a cell needs from the LOD that
// holds the sample into a LaneLod (selects from SGPRs), then compute the cell ONCE per sample: the six clamps and wraps
// are not repeated per LOD of the cascade.
#pragma once

#include "ray_common.h"

namespace svr_linear {

using svr_common::wrap;

// What a cell needs from the LOD that holds the sample, per lane.  The zero state (no LOD holds the sample) gives the
// eight corners the element offset 0: a gather nobody reads, from a valid address.
struct LaneLod {
    int32_t  off[3];           // the window's first voxel
    int32_t  last[3];          // shape - 1
    uint32_t wrap0[3];
    uint32_t ring[3];
    float    s[3];             // the sample in this LOD's voxel units: d * scale
};

__device__ __forceinline__ LaneLod lane_lod_zero() {
    LaneLod q;
#pragma unroll
    for (int a = 0; a < 3; ++a) { q.off[a] = 0; q.last[a] = 0; q.wrap0[a] = 0u; q.ring[a] = 0u; q.s[a] = 0.0f; }
    return q;
}

// Lod: SliceLod / CompLod / IsoLod (the same five fields in each).  s: d * scale of the sample, as the LOD test formed it.
template <class Lod>
__device__ __forceinline__ void lane_lod_take(LaneLod& q, const Lod& L, float sx, float sy, float sz) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q.off[a] = L.off[a]; q.last[a] = (int32_t)L.shape[a] - 1; q.wrap0[a] = L.wrap0[a]; q.ring[a] = L.ring[a];
    }
    q.s[0] = sx; q.s[1] = sy; q.s[2] = sz;
}

struct Cell {
    uint32_t w0[3], w1[3];     // ring slots of the lower / upper corner per axis (clamped to the window, then wrapped)
    float    f[3];
};

__device__ __forceinline__ Cell cell_of(const LaneLod& q) {
    Cell c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = q.s[a] - 0.5f;
        const float b = floorf(p);                     // not a cast: p is negative in the first half voxel
        c.f[a] = p - b;
        const int t0 = (int)b - q.off[a];              // relative to the window: the held sample's own voxel is t0 or t0 + 1
        const int c0 = min(max(t0, 0), q.last[a]);
        const int c1 = min(max(t0 + 1, 0), q.last[a]);
        c.w0[a] = wrap((uint32_t)c0, q.wrap0[a], q.ring[a]);
        c.w1[a] = wrap((uint32_t)c1, q.wrap0[a], q.ring[a]);
    }
    return c;
}

// Element offsets of the corners, index = 4 z + 2 y + x, each from its own wrapped slots (a pair can straddle the
// ring's seam, or two micro-blocks, on any axis).
__device__ __forceinline__ void row_offsets(const LaneLod& q, const Cell& c, size_t o[8]) {
    const size_t rx = q.ring[0], ry = q.ring[1];
    const size_t zy[4] = { ((size_t)c.w0[2] * ry + c.w0[1]) * rx, ((size_t)c.w0[2] * ry + c.w1[1]) * rx,
                           ((size_t)c.w1[2] * ry + c.w0[1]) * rx, ((size_t)c.w1[2] * ry + c.w1[1]) * rx };
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[2 * k] = zy[k] + c.w0[0]; o[2 * k + 1] = zy[k] + c.w1[0]; }
}

__device__ __forceinline__ void blocked_offsets(int esh, const LaneLod& q, const Cell& c, size_t o[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
        o[k] = svr_blocked_index(esh, q.ring[0], q.ring[1], (k & 1) ? c.w1[0] : c.w0[0], (k & 2) ? c.w1[1] : c.w0[1],
                                 (k & 4) ? c.w1[2] : c.w0[2]);
}

// x first, then y, then z, each as a + f * (b - a); v index = 4 z + 2 y + x
__device__ __forceinline__ float blend(const float v[8], const float f[3]) {
    const float c00 = v[0] + f[0] * (v[1] - v[0]);
    const float c10 = v[2] + f[0] * (v[3] - v[2]);
    const float c01 = v[4] + f[0] * (v[5] - v[4]);
    const float c11 = v[6] + f[0] * (v[7] - v[6]);
    const float c0 = c00 + f[1] * (c10 - c00);
    const float c1 = c01 + f[1] * (c11 - c01);
    return c0 + f[2] * (c1 - c0);
}

}  // namespace svr_linear
