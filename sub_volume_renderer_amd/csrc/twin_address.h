// Address of a voxel's texel in the micro-block copy of a ring (svr_lod_desc::blocked_twin; the layout's definition is
// svr_blocked_index): 128-byte blocks of 2^XB x 2^YB x 2^ZB slots in [bz][by][bx] order, the slots of a block in
// [z][y][x] order.  Plain C++ with a portable body for every device builtin: tests/test_twin_address.py compiles it on
// its own with the host compiler and sweeps whole rings against the definition.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVR_TWIN_FN __host__ __device__ __forceinline__
#else
#define SVR_TWIN_FN static inline
#endif

// SY, SZ: log2 of the byte strides of y and z inside a block (ESH = log2 of the element size)
template <int ESH> struct TwinBlock {
    static constexpr int XB = ESH == 0 ? 3 : 2, YB = 2, ZB = ESH == 2 ? 1 : 2, SY = XB + ESH, SZ = XB + YB + ESH;
};

// The march gathers for a lane whose ring slot is voxel + (kx, ky, kz), the constants multiples of the ring extents and
// therefore of the block extents: the slot's block coordinates are the voxel's (bx, by, bz) = (x >> XB, y >> YB, z >> ZB)
// plus constants, its place inside the block is the voxel's own low bits.  With NBx, NBy blocks per ring row and column
// and Kb the block number of the constants,
//   offset = 128 * ((bz * NBy + by) * NBx + bx + Kb) + ((z & zm) << SZ) + ((y & 3) << SY) + ((x & xm) << ESH)
// (all mod 2^32).  Per axis a block index and the low bits that go with it are one linear term in the coordinate and
// the block index — 128 * bx + ((x & xm) << ESH) = (x << ESH) + bx * (128 - (2^XB << ESH)), y and z likewise — so the
// layout is separable:
//   offset = (x << ESH) + (y << SY) + (z << SZ) + (x & ~xm) * Cx + ((Wy * by + Wz * bz + K') << SZ)
//   Cx = (128 >> XB) - (1 << ESH)                    (15, 30, 28 for ESH 0, 1, 2)
//   Wy = (128 * NBx - (4 << SY)) >> SZ               (4 NBx - 1; f32: 2 NBx - 1)
//   Wz = (128 * NBx * NBy - (2^ZB << SZ)) >> SZ      (4 (NBx NBy - 1); f32: 2 (NBx NBy - 1))
//   K' = Kb * (128 >> SZ)                            (per lane, set where the wrap constants change: svr_twin_lane_const)
// From the packed voxel the gather loops hold (x, yz = y | z << 16, y and z below 2^16) that is 6 VALU operations on
// byte rings and 7 on wider ones (x << ESH is one more), where the form above took 9 and more:
//   a   = yz >> (YB, ZB) per 16-bit half             v_pk_lshrrev_b16: by | bz << 16
//   t   = x & ~xm                                    v_and_b32
//   xs  = t * Cx + (x << ESH)                        v_mad_u32_u24 (Cx an inline constant; t < 2^24 like x; + v_lshlrev_b32 where ESH > 0)
//   c   = udot2(yz, 2^SY | 2^SZ << 16, xs)           v_dot2_u32_u16
//   d   = udot2(a, Wy | Wz << 16, K')                v_dot2_u32_u16
//   off = (d << SZ) + c                              v_lshl_add_u32
// It needs Wy and Wz in 16 bits each (svr_twin_separable): byte rings of up to 524,288 slots per plane (1024 x 512).
// Other rings keep the 9-operation form (march_kernel.hip, twin_offset_packed), which reads the same K'; so do float32
// rings for now, whose kernels lost more to the registers of a third gather loop than the shorter address gave back.

// Wy, Wz as defined above (64-bit: the predicate is asked about any ring)
SVR_TWIN_FN uint64_t svr_twin_wy(int esh, uint32_t Rx) {
    const int xb = esh == 0 ? 3 : 2, sy = xb + esh, sz = sy + 2;
    return (128ull * (uint64_t)(Rx >> xb) - (4ull << sy)) >> sz;
}
SVR_TWIN_FN uint64_t svr_twin_wz(int esh, uint32_t Rx, uint32_t Ry) {
    const int xb = esh == 0 ? 3 : 2, sz = xb + esh + 2;
    return (128ull * (uint64_t)(Rx >> xb) * (uint64_t)(Ry >> 2) - 128ull) >> sz;
}
// true where the separable form addresses the copy of a ring of Rx x Ry slots per plane (multiples of 8 x 4)
SVR_TWIN_FN bool svr_twin_separable(int esh, uint32_t Rx, uint32_t Ry) {
    return Rx >= 8u && Ry >= 4u && svr_twin_wy(esh, Rx) <= 0xFFFFull && svr_twin_wz(esh, Rx, Ry) <= 0xFFFFull;
}
// the packed weight word Wy | Wz << 16; 0 where the ring does not qualify (Wy >= 1 on every ring that does)
SVR_TWIN_FN uint32_t svr_twin_weights(int esh, uint32_t Rx, uint32_t Ry) {
    return svr_twin_separable(esh, Rx, Ry) ? (uint32_t)svr_twin_wy(esh, Rx) | ((uint32_t)svr_twin_wz(esh, Rx, Ry) << 16) : 0u;
}
// K' of a lane from the block number of its wrap constants (mod 2^32)
template <int ESH> SVR_TWIN_FN uint32_t svr_twin_lane_const(uint32_t Kb) { return Kb * (128u >> TwinBlock<ESH>::SZ); }

// a.lo * b.lo + a.hi * b.hi + c on 16-bit halves, mod 2^32
SVR_TWIN_FN uint32_t svr_twin_dot2(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short svr_twin_u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_udot2(__builtin_bit_cast(svr_twin_u16x2, a), __builtin_bit_cast(svr_twin_u16x2, b), c, false);
#else
    return (a & 0xFFFFu) * (b & 0xFFFFu) + (a >> 16) * (b >> 16) + c;
#endif
}
// (a.lo >> LO) | (a.hi >> HI) << 16
template <int LO, int HI> SVR_TWIN_FN uint32_t svr_twin_shr2(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short svr_twin_u16x2 __attribute__((ext_vector_type(2)));
    const svr_twin_u16x2 sh = { (unsigned short)LO, (unsigned short)HI };
    return __builtin_bit_cast(uint32_t, (svr_twin_u16x2)(__builtin_bit_cast(svr_twin_u16x2, a) >> sh));
#else
    return ((a & 0xFFFFu) >> LO) | ((a >> 16) >> HI) << 16;
#endif
}

// Byte offset of voxel (x, yz = y | z << 16) in the copy: w = svr_twin_weights of the ring (not 0), Kp = the lane's K'
template <int ESH> SVR_TWIN_FN uint32_t svr_twin_offset(uint32_t x, uint32_t yz, uint32_t w, uint32_t Kp) {
    typedef TwinBlock<ESH> B;
    constexpr uint32_t xm = (1u << B::XB) - 1u, cx = (128u >> B::XB) - (1u << ESH);
    const uint32_t a = svr_twin_shr2<B::YB, B::ZB>(yz);
    const uint32_t t = x & ~xm;
    // (the multiply-add first, as the dot product's addend: the compiler keeps v_mad_u32_u24 and v_lshl_add_u32 whole — with
    //  the product added last it emits v_mul_u32_u24, v_lshlrev_b32 and a v_add3_u32, one operation more)
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t xs = __umul24(t, cx) + (x << ESH);
#else
    const uint32_t xs = t * cx + (x << ESH);
#endif
    const uint32_t c = svr_twin_dot2(yz, (1u << B::SY) | (1u << B::SZ) << 16, xs);
    const uint32_t d = svr_twin_dot2(a, w, Kp);
    return (d << B::SZ) + c;
}
