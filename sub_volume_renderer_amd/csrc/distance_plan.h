// The host plan of svr_distance (include/svr.h; kernels: distance_kernels.hip): how the voxels of a box are indexed and
// how the context's scratch memory is laid out.
//
// Plain C++ on plain integers, so that a test can compile it without HIP (tests/test_distance.py): svr_distance sizes the
// scratch from this plan and svr_launch_distance takes extents, counts and offsets from it, and nowhere else.
//
// Layout.  Voxel (rx, ry, rz) of a box of n voxels per axis has the dense index i = (rz n_y + ry) n_x + rx < 2^30; row
// (ry, rz) has the number rz n_y + ry.
//   bits    one bit per voxel, set where the voxel is a SOURCE, in u32 words along x: wpr words per row.  The init pass
//           reads a row in the units of box_units.h, 4 ring slots at a multiple of 4: voxel rx of a row is element
//           e = rx + head of it, head (0 .. 3; box_head) being the ring slot of the box's first voxel modulo 4.  Bit
//           e & 31 of word e >> 5 of the row belongs to element e, so a unit is one nibble of one word and 8 adjacent
//           lanes make a word with three shuffles, without an atomic.  A row has upr = 8 wpr units; the bits of the
//           elements before the first voxel and behind the last are 0.
//   stack   one DistEntry (distance_scan.h: 8 bytes) per voxel: the stacks of the column pass that is running, entry k
//           of column c at index k * columns + c, so that the lanes of a wave, which hold adjacent columns, touch
//           adjacent entries.  The y pass has n_x n_z columns of n_y entries, the z pass n_x n_y columns of n_z.
// 8 bytes per voxel for the stacks and 1 bit (rounded up to whole words per row) for the sources.  The squared
// distances themselves are worked on in the caller's array.
//
// svr_nearest (NearPlan) works in the same slot and adds, behind the stacks, three planes of owners, one u16 per voxel
// each at the voxel's dense index: own[0] the row voxel rx' of the nearest source of the voxel's row (the x pass), own[1]
// the y' that owns the voxel in its y column (the y pass), own[2] the z' that owns it in its z column (the z pass);
// kDistNoOwner where the row or column has no source.  They are never stored into d2, which the passes rewrite in
// place.  The compose kernel reads them as z' = own[2][z][y][x], y' = own[1][z'][y][x], x' = own[0][z'][y'][x].  6
// bytes per voxel more: 14 bytes and 1 bit per voxel in all.  The x owners are stored, not recomputed from the bits at
// compose time: a plane costs one 2-byte store per voxel in a pass that is bound by its 4-byte store, and the gather
// from it is one load where the row walk is a loop.
#pragma once

#include <stdint.h>

#include "distance_scan.h"

constexpr uint64_t kDistMaxVoxels = 1ull << 30;   // d^2 <= 3 * 2^28 needs the extents, every index in u32 the voxels

struct DistPlan {
    uint32_t n[3];                     // voxels per axis (x, y, z), each <= kDistMaxExtent
    uint32_t voxels;                   // n[0] * n[1] * n[2] <= 2^30
    uint32_t head;                     // elements before a row's first voxel, 0 .. 3
    uint32_t wpr;                      // words of source bits per row
    uint32_t upr;                      // units of 4 ring slots per row: 8 * wpr
    uint32_t units;                    // upr * n[1] * n[2] < 2^32
    uint32_t columns[2];               // of the y pass and of the z pass
    uint64_t bits_off, stack_off;      // byte offsets into the scratch
    uint64_t bytes;                    // of scratch in all
};

// n: the extent of the box, box and window already intersected; head: box_head (box_units.h) of its first voxel.
// false: the box is empty (an n <= 0), has an extent of more than kDistMaxExtent (*refused = 1) or more than
// kDistMaxVoxels voxels (*refused = 2).
inline bool dist_plan(const int64_t n[3], uint32_t head, DistPlan& p, int* refused = nullptr) {
    if (refused) *refused = 0;
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) return false;
    uint64_t voxels = 1;
    for (int a = 0; a < 3; ++a) {
        if ((uint64_t)n[a] > kDistMaxExtent) { if (refused) *refused = 1; return false; }
        voxels *= (uint64_t)n[a];
        p.n[a] = (uint32_t)n[a];
    }
    if (voxels > kDistMaxVoxels) { if (refused) *refused = 2; return false; }
    p.voxels = (uint32_t)voxels;
    p.head = head;
    p.wpr = (p.n[0] + head + 31u) / 32u;
    p.upr = 8u * p.wpr;
    // rows <= 2^28 of at most 16 units where n_x < 30, else upr <= n_x: below 2^32 either way
    p.units = p.upr * p.n[1] * p.n[2];
    p.columns[0] = p.n[0] * p.n[2];
    p.columns[1] = p.n[0] * p.n[1];
    p.bits_off = 0;
    const uint64_t bits = (uint64_t)p.wpr * p.n[1] * p.n[2] * 4u;
    p.stack_off = (bits + 15u) & ~(uint64_t)15u;
    p.bytes = p.stack_off + voxels * sizeof(DistEntry);
    return true;
}

// svr_nearest's: the plan of svr_distance and the three owner planes behind its scratch
struct NearPlan {
    DistPlan d;
    uint64_t own_off[3];               // byte offsets of the x, y and z owners: voxels * 2 bytes each
    uint64_t bytes;                    // of scratch in all: >= d.bytes, the slot is svr_distance's
};

// as dist_plan, which decides what is empty and what is refused
inline bool near_plan(const int64_t n[3], uint32_t head, NearPlan& p, int* refused = nullptr) {
    if (!dist_plan(n, head, p.d, refused)) return false;
    uint64_t at = (p.d.bytes + 15u) & ~(uint64_t)15u;
    for (int a = 0; a < 3; ++a) {
        p.own_off[a] = at;
        at += ((uint64_t)p.d.voxels * sizeof(uint16_t) + 15u) & ~(uint64_t)15u;
    }
    p.bytes = at;
    return true;
}

// The squared distance of voxel r (0 <= r < n) of a row to the nearest source of the row, or kDistFar: the x pass.
// words: the row's wpr words of source bits; e = r + head.  Walks outwards word by word, bounded by the row.  AT: and
// into *at the element of that source: of two at the same distance the left one (the smaller element), e itself where e
// is a source, untouched with kDistFar; else `at` is not used.
template <bool AT>
DIST_FN int32_t dist_row_walk(const uint32_t* words, uint32_t wpr, uint32_t e, uint32_t* at) {
    const uint32_t wi = e >> 5, b = e & 31u;
    const uint32_t w = words[wi];
    if ((w >> b) & 1u) { if (AT) *at = e; return 0; }
    uint32_t best = 0xFFFFFFFFu, where = 0u;
    uint32_t m = w & ((1u << b) - 1u);                                   // the bits below b
    for (uint32_t k = wi;;) {
        if (m) {
            where = 32u * k + 31u - (uint32_t)__builtin_clz(m);
            best = e - where;
            break;
        }
        if (k == 0u) break;
        m = words[--k];
    }
    m = b == 31u ? 0u : (w & (0xFFFFFFFFu << (b + 1u)));                 // the bits above b
    for (uint32_t k = wi;;) {
        if (m) {
            const uint32_t right = 32u * k + (uint32_t)__builtin_ctz(m);
            if (right - e < best) { best = right - e; where = right; }   // strictly nearer: a tie stays left
            break;
        }
        if (++k == wpr) break;
        m = words[k];
    }
    if (best == 0xFFFFFFFFu) return kDistFar;
    if (AT) *at = where;
    return (int32_t)(best * best);
}

// svr_distance's x pass, and svr_nearest's
DIST_FN int32_t dist_row_nearest(const uint32_t* words, uint32_t wpr, uint32_t e) { return dist_row_walk<false>(words, wpr, e, nullptr); }
DIST_FN int32_t dist_row_nearest_at(const uint32_t* words, uint32_t wpr, uint32_t e, uint32_t* at) { return dist_row_walk<true>(words, wpr, e, at); }
