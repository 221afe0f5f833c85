// What the three box passes share (mesh_kernels.hip, components_kernels.hip, distance_kernels.hip).  A pass reads a box
// of one LOD's resident window row by row in units of 4 ring slots at a multiple of 4, decides for every voxel whether
// it is inside, and counts.  Element e = rx + head of a row belongs to voxel rx, head (0 .. 3) being the ring slot of
// the box's first voxel modulo 4, so a unit whole inside the row that the ring's wrap seam does not cut is one aligned
// load of 16 bytes (8 of a u16 ring, 4 of a u8 ring).  The host half is plain C++ on plain integers, which the plan
// headers include and the tests compile without HIP.  The device half (under __HIPCC__) is what the first kernel of
// each chain does with a unit; each kernel keeps its own loop over the units and its own sink.
#pragma once

#include <stdint.h>

// the ring slot modulo 4 of the box's first voxel (lo_x >= 0: a window offset is never negative)
inline uint32_t box_head(int64_t lo_x, uint32_t ring_x) { return (uint32_t)(lo_x % (int64_t)ring_x) & 3u; }

#ifdef __HIPCC__
#include "ring_pieces.h"

// 4 elements at an address that is a multiple of 4 elements, as floats
template <typename T> struct BoxElem;
template <> struct BoxElem<uint8_t> {
    static __device__ __forceinline__ void load4(const uint8_t* p, float v[4]) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
        v[0] = (float)(q & 0xFFu); v[1] = (float)((q >> 8) & 0xFFu); v[2] = (float)((q >> 16) & 0xFFu); v[3] = (float)(q >> 24);
    }
};
template <> struct BoxElem<uint16_t> {
    static __device__ __forceinline__ void load4(const uint16_t* p, float v[4]) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = (float)(q.x & 0xFFFFu); v[1] = (float)(q.x >> 16); v[2] = (float)(q.y & 0xFFFFu); v[3] = (float)(q.y >> 16);
    }
};
template <> struct BoxElem<float> {
    static __device__ __forceinline__ void load4(const float* p, float v[4]) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};

// ring slot of voxel r (0 <= r < n <= ring) of the box on one axis
__device__ __forceinline__ uint32_t box_slot(uint32_t s0, uint32_t r, uint32_t ring) {
    const uint32_t s = s0 + r;
    return s >= ring ? s - ring : s;
}

// element offset of the row (ry, rz) of the box in the ring: 64-bit, a ring may hold 2^32 elements or more.  Args: any
// kernel-argument struct with ring[3] (the ring's extents) and s0[3] (the ring slot of the box's first voxel).
template <class Args>
__device__ __forceinline__ size_t box_row_offset(const Args& a, uint32_t ry, uint32_t rz) {
    const uint32_t sy = box_slot(a.s0[1], ry, a.ring[1]), sz = box_slot(a.s0[2], rz, a.ring[2]);
    return ((size_t)sz * a.ring[1] + sy) * (size_t)a.ring[0];
}

// The rest are macros, as RING_WALK is (ring_pieces.h) and for its reason: behind functions, whatever their signatures,
// the init kernels were no longer the code objects they were when each spelt these lines out (profiles/box_units/).
// The unit at voxels r0 .. r0 + 3 of the row at rowoff (r0 may be negative and r0 + 3 beyond the row): LEVEL the values
// of the density ring into val[4], else the labels into lab[4] (untouched without a label ring), and into `have`, 0
// before, bit j where voxel r0 + j lies in the row.  One aligned load where the unit is whole, inside the row and
// aligned, else its elements one by one (a row's head and tail, the slot the ring's wrap seam cuts).  a: the kernel's
// arguments, with labels beside what box_row_offset needs; ring = a.density as T; n0 = a.n[0].
#define BOX_GATHER(T, LEVEL, a, ring, n0, rowoff, r0, val, lab, have)                                                 \
    do {                                                                                                              \
        bool whole = (r0) >= 0 && (r0) + 4 <= (int32_t)(n0);                                                          \
        uint32_t sx0 = 0u;                                                                                            \
        if (whole) {                                                                                                  \
            sx0 = box_slot((a).s0[0], (uint32_t)(r0), (a).ring[0]);                                                   \
            whole = sx0 + 4u <= (a).ring[0];                 /* not the slot the wrap seam cuts */                    \
        }                                                                                                             \
        if (whole) {                                                                                                  \
            (have) = 0xFu;                                                                                            \
            if (LEVEL) {                                                                                              \
                const T* const p = (ring) + (rowoff) + sx0;                                                           \
                if ((reinterpret_cast<uintptr_t>(p) & (4u * sizeof(T) - 1u)) == 0u) BoxElem<T>::load4(p, (val));      \
                else {                                                                                                \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j) (val)[j] = (float)p[j];                             \
                }                                                                                                     \
            } else if ((a).labels) {                                                                                  \
                const uint32_t* const p = (a).labels + (rowoff) + sx0;                                                \
                if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0u) {                                                   \
                    const uint4 q = *reinterpret_cast<const uint4*>(p);                                               \
                    (lab)[0] = q.x; (lab)[1] = q.y; (lab)[2] = q.z; (lab)[3] = q.w;                                   \
                } else {                                                                                              \
                    _Pragma("unroll") for (int j = 0; j < 4; ++j) (lab)[j] = p[j];                                    \
                }                                                                                                     \
            }                                                                                                         \
        } else {                                                                                                      \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                           \
                const int32_t r = (r0) + j;                                                                           \
                if (r >= 0 && r < (int32_t)(n0)) {                                                                    \
                    (have) |= 1u << j;                                                                                \
                    const size_t e = (rowoff) + box_slot((a).s0[0], (uint32_t)r, (a).ring[0]);                        \
                    if (LEVEL) (val)[j] = (float)(ring)[e];                                                           \
                    else if ((a).labels) (lab)[j] = (a).labels[e];                                                    \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
    } while (0)

// in = inside(): LEVEL the value reaches the level (a NaN is outside); else `selected`, the search of the label in the
// pass's list as the pass words it (the mesh searches a list that is never empty; to the others an empty one selects
// all), evaluated only when the label differs from the lane's last (c: its BoxInside, started as {}): neighbours mostly
// share theirs.  `...`: what a pass with ignore_zero does to `in` then, BOX_DROP_ZERO; the mesh: nothing.
struct BoxInside {
    uint32_t last_label;
    bool last_in, have_last;
};
#define BOX_INSIDE(in, LEVEL, c, val, lab, level, selected, ...)                                                      \
    if (LEVEL) (in) = (val) >= (level);                                                                               \
    else {                                                                                                            \
        if (!(c).have_last || (lab) != (c).last_label) { (c).last_in = (selected); (c).last_label = (lab); (c).have_last = true; }\
        (in) = (c).last_in;                                                                                           \
        __VA_ARGS__                                                                                                   \
    }
// a selected voxel of label 0 is outside, and counted
#define BOX_DROP_ZERO(in, lab, ignore_zero, zeros) if ((in) && (ignore_zero) && (lab) == 0u) { (in) = false; ++(zeros); }

// The lanes' counters v and w summed over their wave and added to the header: an atomic per wave and word, none for a 0
#define BOX_WAVE_ADD2(word_v, v, word_w, w)                                                                           \
    do {                                                                                                              \
        _Pragma("unroll") for (int d = 32; d >= 1; d >>= 1) {                                                         \
            (v) += (uint32_t)__shfl_xor((int)(v), d);                                                                 \
            (w) += (uint32_t)__shfl_xor((int)(w), d);                                                                 \
        }                                                                                                             \
        if (__lane_id() == 0u) {                                                                                      \
            if (v) atomicAdd((word_v), (unsigned long long)(v));                                                      \
            if (w) atomicAdd((word_w), (unsigned long long)(w));                                                      \
        }                                                                                                             \
    } while (0)
#define BOX_WAVE_ADD(word, v) do { uint32_t none = 0u; BOX_WAVE_ADD2(word, v, word, none); } while (0)

#endif  // __HIPCC__
