// The faces of svr_contacts (include/svr.h; kernel: contacts_kernels.hip) as one unit of 4 voxels sees them: the key of
// an unordered label pair, its hash, and the function that turns a unit and its three neighbourhoods (the voxel after
// it in x, the 4 voxels of row y + 1, the 4 of row z + 1) into merged face updates.  Plain C++ on plain integers with
// static indexing only, shared by the kernel and by a host program that holds it to brute force (tests/test_contacts.py).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define CON_HD __host__ __device__ __forceinline__
#define CON_UNROLL _Pragma("unroll")
#else
#define CON_HD inline
#define CON_UNROLL
#endif

constexpr uint32_t kConUnit = 4;            // voxels of a unit: 4 consecutive ring slots at a multiple of 4

// The first 8 bytes of a record as one little-endian u64: label_lo in the low word, label_hi in the high one.  hi >= 1
// for every face (lo < hi), so the key of a face is never 0.
CON_HD uint64_t con_key(uint32_t a, uint32_t b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
CON_HD uint32_t con_key_lo(uint64_t key) { return (uint32_t)key; }
CON_HD uint32_t con_key_hi(uint64_t key) { return (uint32_t)(key >> 32); }

CON_HD uint32_t con_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// both labels reach every bit: the pairs of one object with its many neighbours spread like unrelated ones
CON_HD uint32_t con_hash(uint64_t key) { return con_mix(con_key_lo(key) ^ (con_mix(con_key_hi(key)) * 0x9E3779B1u)); }

// A unit: its 4 labels, bit j of `have` where voxel j lies in the box's row; the label after voxel 3 in x and whether
// that voxel exists; the labels of the same 4 x in row y + 1 and in row z + 1 with their masks (0: no such row).
struct ConUnit {
    uint32_t lab[4], have;
    uint32_t xlab, xhave;
    uint32_t ylab[4], yhave;
    uint32_t zlab[4], zhave;
};

// the faces between lab[j] and nb[j] -> bit j where both exist and differ, key[j] their pair (0 without a face)
CON_HD uint32_t con_axis_faces(const uint32_t lab[4], uint32_t have, const uint32_t nb[4], uint32_t nbhave, uint64_t key[4]) {
    uint32_t fm = 0u;
    CON_UNROLL for (int j = 0; j < 4; ++j) {
        const bool face = ((have & nbhave) >> j & 1u) && lab[j] != nb[j];
        key[j] = face ? con_key(lab[j], nb[j]) : 0ull;
        if (face) fm |= 1u << j;
    }
    return fm;
}

// the faces of the three axes, keys dropped: does the unit own any face at all?
CON_HD bool con_unit_any(const ConUnit& u) {
    const uint32_t xnb[4] = {u.lab[1], u.lab[2], u.lab[3], u.xlab};
    const uint32_t xnbhave = (u.have >> 1) | ((u.xhave & 1u) << 3);
    uint32_t any = 0u;
    CON_UNROLL for (int j = 0; j < 4; ++j) {
        const uint32_t own = u.have >> j & 1u;
        any |= own & (xnbhave >> j & 1u) & (uint32_t)(u.lab[j] != xnb[j]);
        any |= own & (u.yhave >> j & 1u) & (uint32_t)(u.lab[j] != u.ylab[j]);
        any |= own & (u.zhave >> j & 1u) & (uint32_t)(u.lab[j] != u.zlab[j]);
    }
    return any != 0u;
}

// The lowest pending face of fm (not 0) and every later one of the same pair leave fm as one update -> their mask,
// k their key.  Static indexing only: the keys stay in registers.
CON_HD uint32_t con_take(const uint64_t key[4], uint32_t& fm, uint64_t& k) {
    k = (fm & 1u) ? key[0] : (fm & 2u) ? key[1] : (fm & 4u) ? key[2] : key[3];
    uint32_t m = 0u;
    CON_UNROLL for (int j = 0; j < 4; ++j)
        if ((fm >> j & 1u) && key[j] == k) m |= 1u << j;
    fm &= ~m;
    return m;
}

// The merged face updates of a unit: keep(key) is asked once per face, in the order x, y, z and by ascending voxel,
// and the faces it keeps go to sink(axis, key, mask), one call per axis and distinct pair, bit j of mask: the face is
// owned by voxel j.  Count, coordinate sums and extremes of an update are arithmetic on the mask.
template <class Keep, class Sink>
CON_HD void con_unit_updates(const ConUnit& u, Keep&& keep, Sink&& sink) {
    const uint32_t xnb[4] = {u.lab[1], u.lab[2], u.lab[3], u.xlab};
    const uint32_t xnbhave = (u.have >> 1) | ((u.xhave & 1u) << 3);
    CON_UNROLL for (int axis = 0; axis < 3; ++axis) {
        uint64_t key[4];
        uint32_t fm = axis == 0 ? con_axis_faces(u.lab, u.have, xnb, xnbhave, key)
                    : axis == 1 ? con_axis_faces(u.lab, u.have, u.ylab, u.yhave, key)
                                : con_axis_faces(u.lab, u.have, u.zlab, u.zhave, key);
        CON_UNROLL for (int j = 0; j < 4; ++j)
            if ((fm >> j & 1u) && !keep(key[j])) fm &= ~(1u << j);
        while (fm) {
            uint64_t k;
            const uint32_t m = con_take(key, fm, k);
            sink(axis, k, m);
        }
    }
}

// what the mask of an update stands for: its faces, the sum of the owning voxels' positions 0 .. 3, the first and last
CON_HD uint32_t con_mask_count(uint32_t m) { return (m & 1u) + (m >> 1 & 1u) + (m >> 2 & 1u) + (m >> 3 & 1u); }
CON_HD uint32_t con_mask_sum(uint32_t m) { return (m >> 1 & 1u) + 2u * (m >> 2 & 1u) + 3u * (m >> 3 & 1u); }
CON_HD uint32_t con_mask_first(uint32_t m) { return (m & 1u) ? 0u : (m & 2u) ? 1u : (m & 4u) ? 2u : 3u; }
CON_HD uint32_t con_mask_last(uint32_t m) { return (m & 8u) ? 3u : (m & 4u) ? 2u : (m & 2u) ? 1u : 0u; }

// The walk over a box of n[0] x n[1] x n[2] voxels whose first voxel sits `head` (0 .. 3) elements into its unit:
// units per row, units in all, and the contiguous share of whole steps (of `step` units) that each of at most
// `most_groups` workgroups takes, at least `min_steps` steps.  -> the workgroups
struct ConPlan { uint32_t head, upr; uint64_t units, share; uint32_t blocks; };
inline ConPlan con_plan(const int64_t n[3], uint32_t head, uint32_t step, uint32_t min_steps, uint64_t most_groups) {
    ConPlan p;
    p.head = head;
    p.upr = (uint32_t)((head + (uint64_t)n[0] + kConUnit - 1u) / kConUnit);
    p.units = (uint64_t)p.upr * (uint64_t)n[1] * (uint64_t)n[2];
    uint64_t share = (p.units + most_groups - 1u) / most_groups;
    share = (share + step - 1u) / step * step;
    if (share < (uint64_t)step * min_steps) share = (uint64_t)step * min_steps;
    p.share = share;
    p.blocks = (uint32_t)((p.units + share - 1u) / share);
    return p;
}
