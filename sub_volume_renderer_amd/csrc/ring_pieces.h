// The one statement of how a streaming pass walks a box of one LOD's resident window (histogram_kernels.hip,
// object_kernels.hip): box and window, already intersected, are cut at the ring's wrap seams into at most 2 x 2 x 2
// dense pieces of the row-major ring, and whole rows of a piece are dealt to workgroups; 2^k lanes share a row, which
// they read in 16-byte slots.
//
// The host half is plain C++ on plain integers, so that a test can compile it without HIP (tests/test_ring_pieces.py):
// the launchers decide the pieces here and nowhere else.  The device half (under __HIPCC__) is what the kernels do with
// a plan: find the workgroup's piece and rows, address a row; and what both passes need besides, the u32 keys that
// order like floats and the search of a sorted id list.
#pragma once

#include <stdint.h>

constexpr int kRingMaxPieces = 8;

// A piece in two parts, where it lies and how its rows are dealt out: a pass that carries more per piece puts it
// between the two (object_kernels.hip: ObjPiece)
struct RingBox {
    uint32_t s[3];             // first ring slot (x, y, z)
    uint32_t n[3];             // extent; s + n <= ring on every axis
};
struct RingShare {
    uint32_t rows;             // n[1] * n[2]
    uint32_t rows_per_wg;      // rows_per_wg * n[0] < 2^32: a workgroup may count its voxels in u32
    uint32_t block0;           // first workgroup of this piece
    uint32_t lpr_log2;         // log2 of the lanes that share a row
    uint32_t spr;              // 16-byte slots a row can touch
};
struct RingPiece : RingBox, RingShare {};

// what a kernel receives
struct RingPieces {
    int32_t npieces;
    RingPiece piece[kRingMaxPieces];
};

struct RingPlan {
    RingPieces pieces;
    uint32_t rel[kRingMaxPieces][3];   // logical coordinate of a piece's first voxel, relative to the window offset
    uint32_t blocks;                   // workgroups in all
};

// what a pass reads and how it is sized
struct RingPass {
    uint32_t bytes_per_voxel;  // read per voxel: what a workgroup's share is measured in
    uint32_t per_slot;         // voxels per 16-byte slot (16, 8 or 4)
    uint64_t slot_base;        // address of the ring whose 16-byte groups are the slots (its elements have
                               // 16 / per_slot bytes); 0 where there is no such ring: groups of per_slot element indices
    uint64_t workgroups;       // the grid to size for, over the whole box
    uint64_t min_share;        // bytes a workgroup reads at least
};

// lo[a] .. lo[a] + n[a]: logical voxels of the LOD inside its window (n > 0, n <= ring); off: the window offset.
// false: more rows or workgroups than 32 bits hold (not with int32 ring extents below 2^16 x 2^16 rows).
inline bool ring_plan(const uint32_t ring[3], const int32_t off[3], const int64_t lo[3], const int64_t n[3], const RingPass& pass,
                      RingPlan& plan) {
    // per axis the run up to the ring's end, then the run that wrapped to its start
    uint32_t s[3][2], m[3][2]; int cnt[3];
    uint64_t total = 1;
    for (int ax = 0; ax < 3; ++ax) {
        const uint32_t R = ring[ax];
        int64_t s64 = lo[ax] % (int64_t)R;
        if (s64 < 0) s64 += R;
        const uint32_t s0 = (uint32_t)s64, len = (uint32_t)n[ax];
        const uint32_t first = len < R - s0 ? len : R - s0;
        s[ax][0] = s0; m[ax][0] = first; cnt[ax] = 1;
        if (first < len) { s[ax][1] = 0u; m[ax][1] = len - first; cnt[ax] = 2; }
        total *= (uint64_t)len;
    }
    uint64_t bytes_per_wg = total * pass.bytes_per_voxel / pass.workgroups;
    if (bytes_per_wg < pass.min_share) bytes_per_wg = pass.min_share;
    // Rows start (slot_base / es + s[0] + k ring[0]) mod per_slot elements into a slot, k counting the ring's rows:
    // `step` apart, the largest power of two that divides ring[0] and per_slot
    const uint32_t per_slot = pass.per_slot, es = 16u / per_slot;
    const uint32_t both = ring[0] | per_slot, step = both & (0u - both);
    plan.blocks = 0;
    plan.pieces.npieces = 0;
    for (int iz = 0; iz < cnt[2]; ++iz)
        for (int iy = 0; iy < cnt[1]; ++iy)
            for (int ix = 0; ix < cnt[0]; ++ix) {
                const int pi = plan.pieces.npieces++;
                RingPiece& P = plan.pieces.piece[pi];
                const int idx[3] = {ix, iy, iz};
                for (int ax = 0; ax < 3; ++ax) {
                    P.s[ax] = s[ax][idx[ax]]; P.n[ax] = m[ax][idx[ax]];
                    plan.rel[pi][ax] = (uint32_t)(lo[ax] - (int64_t)off[ax]) + (idx[ax] ? m[ax][0] : 0u);
                }
                const uint64_t rows = (uint64_t)P.n[1] * P.n[2];
                if (rows > 0xFFFFFFFFull) return false;
                P.rows = (uint32_t)rows;
                const uint64_t row_bytes = (uint64_t)P.n[0] * pass.bytes_per_voxel;
                uint64_t rpw = (bytes_per_wg + row_bytes - 1) / row_bytes;
                const uint64_t cap = 0xFFFFFFFFull / P.n[0];
                if (rpw > cap) rpw = cap;
                if (rpw > rows) rpw = rows;
                if (rpw < 1) rpw = 1;
                P.rows_per_wg = (uint32_t)rpw;
                // slots per row: the row and the most elements that come before one in its first slot
                const uint32_t head0 = (uint32_t)((pass.slot_base / es + P.s[0]) % per_slot);
                const uint32_t head = per_slot - step + head0 % step;
                P.spr = (uint32_t)(((uint64_t)head + P.n[0] + per_slot - 1u) / per_slot);
                // lanes per row: the power of two that covers the slots, or for longer rows the one (at least 8
                // lanes: whole 128-byte lines) whose multiple wastes the fewest lanes
                uint32_t lg = 0;
                while (lg < 3u && (1u << lg) < P.spr) ++lg;
                if (P.spr > 8u) {
                    uint32_t best = 0xFFFFFFFFu;
                    for (uint32_t g = 3u; g <= 8u; ++g) {
                        const uint32_t padded = ((P.spr + (1u << g) - 1u) >> g) << g;
                        if (padded <= best) { best = padded; lg = g; }
                    }
                }
                P.lpr_log2 = lg;
                P.block0 = plan.blocks;
                const uint64_t nb = (rows + rpw - 1) / rpw;
                if (nb + plan.blocks > 0x7FFFFFFFull) return false;
                plan.blocks += (uint32_t)nb;
            }
    return true;
}

#ifdef __HIPCC__

// the grid a pass sizes its shares for: per_cu workgroups on every CU of the device
inline uint64_t ring_workgroups(int device, uint64_t per_cu) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
    return (uint64_t)cus * per_cu;
}

// u32 keys that order like the floats they come from (never given a NaN)
__device__ __forceinline__ uint32_t ring_key_of_float(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ring_float_of_key(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// lower-bound search; every probe lies in [0, n) whatever the order of `s` (outline_kernel's)
__device__ __forceinline__ bool ring_in_set(const uint32_t* __restrict__ s, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && s[lo] == v;
}

// The prologue of a workgroup of THREADS threads (ps: npieces and piece[] among its kernel arguments), declared into
// the kernel's scope: its piece P = ps.piece[pi] and the rows [r0, r1) it takes of it, rows_per_iter at a time; lpr
// lanes share a row, this one takes slots lane_slot + k * lpr of row rb + lane_row.  Wave-uniform but for lane_row and
// lane_slot.  A macro, as RING_ROW_OFFSET is, so that it serves any piece type and the kernels stay the code objects
// they were when each spelt these lines out (profiles/ring_pieces/kernel_diff.txt).
#define RING_WALK(THREADS, ps, block, tid)                                                                  \
    int pi = 0;                                                                                             \
    while (pi + 1 < (ps).npieces && (block) >= (ps).piece[pi + 1].block0) ++pi;                             \
    const auto& P = (ps).piece[pi];                                                                         \
    const uint32_t r0 = ((block) - P.block0) * P.rows_per_wg;                                               \
    const uint32_t r1 = (uint32_t)min((uint64_t)P.rows, (uint64_t)r0 + P.rows_per_wg);                      \
    const uint32_t lpr = 1u << P.lpr_log2, rows_per_iter = (THREADS) >> P.lpr_log2;                         \
    const uint32_t lane_row = (tid) >> P.lpr_log2, lane_slot = (tid) & (lpr - 1u)

// element offset of row (ry, rz) of piece P in a ring of extents ring[3]: 64-bit, a ring may hold 2^32 elements or more
#define RING_ROW_OFFSET(P, ring, ry, rz) \
    (((size_t)((P).s[2] + (rz)) * (size_t)(ring)[1] + (size_t)((P).s[1] + (ry))) * (size_t)(ring)[0] + (size_t)(P).s[0])

#endif  // __HIPCC__
