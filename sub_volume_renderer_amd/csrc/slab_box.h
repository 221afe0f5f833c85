// The bounding box of a wave's samples over one brick slab (march_kernel.hip, "LDS brick slabs"), reduced over the 64
// lanes as packed 16-bit minima.  Plain C++ with a portable body for every device builtin: tests/test_slab_box.py
// compiles it on its own with the host compiler.
//
// Voxel indices of live lanes lie inside the LOD's window, [off, off + shape) per axis.  Where that window lies inside
// [0, 32767] (svr_slab_box_fits16; the host stages bricks on no other LOD), a lower bound l and a negated upper bound
// -h are both signed 16-bit values, and the box of the wave is the lane-wise MINIMUM of three words per lane,
//   A = lx | ly << 16      B = lz | (-hz) << 16      C = (-hx) | (-hy) << 16
// (a maximum is carried as the minimum of the negated values: no bias to add per lane, the sign comes back on the
// scalar side).  A lane that is not live holds SVR_SLAB_BOX_NONE in all three: the largest value of either kind, so it
// never wins, and a wave without a live lane comes out with lx > hx (svr_slab_box::none).
//
// The reduction (svr_slab_box_reduce on the device; tests restate it over 64 array slots in the same order):
//   level 32: one half swap of (A, B) and one packed min leave A's partial minima in lanes 0-31, B's in lanes 32-63
//   level 16: one row swap of (that, C) and one packed min leave, per row of 16 lanes,
//             row 0: A   row 1: C of lanes 0-31   row 2: B   row 3: C of lanes 32-63
//   in a row: four steps of a DPP move and a packed min on that ONE register
// 2 + 2 + 8 vector operations and four lane reads, where six separate 32-bit reductions took 36 and six.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVR_BOX_FN __host__ __device__ __forceinline__
#else
#define SVR_BOX_FN static inline
#endif

#define SVR_SLAB_BOX_NONE 0x7fff7fffu

// 1: the voxel indices of a window [off, off + shape) fit the packed reduction (0 <= index <= 32767); 0: they do not
SVR_BOX_FN bool svr_slab_box_fits16(long long off, long long shape) { return off >= 0 && off + shape <= 32767; }
// What a LOD with these windows does.  PACKED: its boxes are reduced as above.  UNPACKED: they cannot be — and there is NO
// unpacked reduction in the kernel to fall back on: fill_params sets LodParams::slab = 0 for such a LOD, it stages no
// bricks at all and its samples are gathered directly (the packed (y, z) brick address needs the same index range).
enum svr_slab_box_mode { SVR_SLAB_BOX_UNPACKED = 0, SVR_SLAB_BOX_PACKED = 1 };
SVR_BOX_FN svr_slab_box_mode svr_slab_box_mode_of(const int32_t off[3], const uint32_t shape[3]) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = ok && svr_slab_box_fits16(off[a], shape[a]);
    return ok ? SVR_SLAB_BOX_PACKED : SVR_SLAB_BOX_UNPACKED;
}

// lane-wise signed minimum of both 16-bit halves (v_pk_min_i16)
SVR_BOX_FN uint32_t svr_slab_box_min2(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short svr_box_i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(svr_box_i16x2, a), __builtin_bit_cast(svr_box_i16x2, b)));
#else
    const int16_t lo = (int16_t)(a & 0xFFFFu) < (int16_t)(b & 0xFFFFu) ? (int16_t)(a & 0xFFFFu) : (int16_t)(b & 0xFFFFu);
    const int16_t hi = (int16_t)(a >> 16) < (int16_t)(b >> 16) ? (int16_t)(a >> 16) : (int16_t)(b >> 16);
    return (uint32_t)(uint16_t)lo | (uint32_t)(uint16_t)hi << 16;
#endif
}

// the same, maximum (v_pk_max_i16)
SVR_BOX_FN uint32_t svr_slab_box_max2(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short svr_box_i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(svr_box_i16x2, a), __builtin_bit_cast(svr_box_i16x2, b)));
#else
    const int16_t lo = (int16_t)(a & 0xFFFFu) > (int16_t)(b & 0xFFFFu) ? (int16_t)(a & 0xFFFFu) : (int16_t)(b & 0xFFFFu);
    const int16_t hi = (int16_t)(a >> 16) > (int16_t)(b >> 16) ? (int16_t)(a >> 16) : (int16_t)(b >> 16);
    return (uint32_t)(uint16_t)lo | (uint32_t)(uint16_t)hi << 16;
#endif
}

// (int)lo | (int)(NEG ? -hi : hi) << 16 of two floats whose truncations fit 16 signed bits: two converts, the second
// one writes the upper half of the register directly (and negates its source for nothing)
template <bool NEG> SVR_BOX_FN uint32_t svr_slab_box_cvt2(float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r = (uint32_t)(int)lo;
    if (NEG) asm("v_cvt_i32_f32_sdwa %0, -%1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(r) : "v"(hi));
    else asm("v_cvt_i32_f32_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(r) : "v"(hi));
    return r;
#else
    return ((uint32_t)(int)lo & 0xFFFFu) | (uint32_t)(NEG ? -(int)hi : (int)hi) << 16;
#endif
}
// both halves negated (v_pk_sub_i16 from 0)
SVR_BOX_FN uint32_t svr_slab_box_neg2(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short svr_box_i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (svr_box_i16x2)(-__builtin_bit_cast(svr_box_i16x2, a)));
#else
    return ((0u - (a & 0xFFFFu)) & 0xFFFFu) | (0u - (a >> 16)) << 16;
#endif
}

// The three words of one lane from the coordinates (not yet truncated) of its first and last sample of the slab, per
// axis (ic is monotone along a ray: the two bound the rest); `live` false: the lane takes no part.
struct svr_slab_box_words { uint32_t a, b, c; };
SVR_BOX_FN svr_slab_box_words svr_slab_box_pack(float x0, float x1, float y0, float y1, float z0, float z1, bool live) {
    const uint32_t e0 = svr_slab_box_cvt2<false>(x0, y0), e1 = svr_slab_box_cvt2<false>(x1, y1);
    const uint32_t c = svr_slab_box_neg2(svr_slab_box_max2(e0, e1));
    // z: (z0, -z1) against (z1, -z0) gives (lz, -hz) in one packed min
    const uint32_t b = svr_slab_box_min2(svr_slab_box_cvt2<true>(z0, z1), svr_slab_box_cvt2<true>(z1, z0));
    svr_slab_box_words w;
    w.a = live ? svr_slab_box_min2(e0, e1) : SVR_SLAB_BOX_NONE;
    w.b = live ? b : SVR_SLAB_BOX_NONE;
    w.c = live ? c : SVR_SLAB_BOX_NONE;
    return w;
}

// The wave's box from the four reduced words: a = A, b = B, and C in two parts (lanes 0-31 and 32-63), see above
struct svr_slab_box { int lx, ly, lz, hx, hy, hz; bool none; };
SVR_BOX_FN svr_slab_box svr_slab_box_unpack(uint32_t a, uint32_t b, uint32_t c_lo, uint32_t c_hi) {
    svr_slab_box r;
    r.lx = (int)(int16_t)(a & 0xFFFFu); r.ly = (int)a >> 16;
    r.lz = (int)(int16_t)(b & 0xFFFFu); r.hz = -((int)b >> 16);
    const int nhx0 = (int)(int16_t)(c_lo & 0xFFFFu), nhx1 = (int)(int16_t)(c_hi & 0xFFFFu);
    const int nhy0 = (int)c_lo >> 16, nhy1 = (int)c_hi >> 16;
    r.hx = -(nhx0 < nhx1 ? nhx0 : nhx1); r.hy = -(nhy0 < nhy1 ? nhy0 : nhy1);
    r.none = r.lx > r.hx;
    return r;
}

#if defined(__HIPCC__)
// One wave64 (every lane active) reduces the words of its lanes; the result is wave-uniform.
__device__ __forceinline__ svr_slab_box svr_slab_box_reduce(svr_slab_box_words w) {
    // level 32: lanes 32-63 of A change places with lanes 0-31 of B
    const auto s32 = __builtin_amdgcn_permlane32_swap(w.a, w.b, false, false);
    const uint32_t ab = svr_slab_box_min2(s32[0], s32[1]);                // rows: A A B B
    // level 16: rows 1, 3 of that change places with rows 0, 2 of C
    const auto s16 = __builtin_amdgcn_permlane16_swap(ab, w.c, false, false);
    uint32_t r = svr_slab_box_min2(s16[0], s16[1]);                       // rows: A C(0-31) B C(32-63)
    // inside a row: lane ^ 1, lane ^ 2, then the mirrored half row and the mirrored row
    r = svr_slab_box_min2(r, (uint32_t)__builtin_amdgcn_mov_dpp((int)r, 0xB1, 0xf, 0xf, false));     // quad_perm:[1,0,3,2]
    r = svr_slab_box_min2(r, (uint32_t)__builtin_amdgcn_mov_dpp((int)r, 0x4E, 0xf, 0xf, false));     // quad_perm:[2,3,0,1]
    r = svr_slab_box_min2(r, (uint32_t)__builtin_amdgcn_mov_dpp((int)r, 0x141, 0xf, 0xf, false));    // row_half_mirror
    r = svr_slab_box_min2(r, (uint32_t)__builtin_amdgcn_mov_dpp((int)r, 0x140, 0xf, 0xf, false));    // row_mirror
    return svr_slab_box_unpack((uint32_t)__builtin_amdgcn_readlane((int)r, 0), (uint32_t)__builtin_amdgcn_readlane((int)r, 32),
                               (uint32_t)__builtin_amdgcn_readlane((int)r, 16), (uint32_t)__builtin_amdgcn_readlane((int)r, 48));
}
#endif
