// The host plan of svr_split (include/svr.h; kernels: split_kernels.hip): how the context's scratch memory is laid out
// and how many levels the prefix scan over the region seeds has.  Plain C++ on plain integers, so that a test can
// compile it without HIP (tests/test_split.py): svr_split sizes the scratch from this plan and svr_launch_split takes
// extents, counts, scan levels and offsets from it, and nowhere else.
//
// Layout.  Voxel (x, y, z) of a box of n voxels per axis has the dense index i = (z n_y + y) n_x + x < 2^30.
//   up      one u32 per voxel: kSplitOutside for a voxel that is outside, else up(i); after the summit pass summit(i).
//   uf      one u32 per voxel, the union-find of components_uf.h in which only summits are entries: a summit starts as
//           its own root, every other voxel holds kSplitOutside for good.  After the flatten pass a summit holds the
//           seed of its region.
//   aux     one u32 per voxel, written at seeds only: the rank of the region (its number minus one).
//   scan    level 0 holds one u32 per block of kBoxScanBlock voxels, the seeds among them; the levels above it are
//           those of box_scan.h.
// 12 bytes per voxel, and 4 bytes per 256 voxels for the scan.
#pragma once

#include <stdint.h>

#include "box_scan.h"
#include "box_units.h"

constexpr uint32_t kSplitOutside = 0xFFFFFFFFu;    // == kUfOutside (components_uf.h)
constexpr uint64_t kSplitMaxVoxels = 1ull << 30;   // SVR_SPLIT_MAX_VOXELS
constexpr uint32_t kSplitMaxMerge = 1u << 29;      // SVR_SPLIT_MAX_MERGE

struct SplitPlan {
    uint32_t n[3];                     // voxels per axis (x, y, z)
    uint32_t voxels;                   // n[0] * n[1] * n[2] <= 2^30: every index, and kSplitOutside beside them, fits u32
    uint64_t up_off, uf_off, aux_off;  // byte offsets into the scratch
    BoxScanPlan scan;                  // count[0] = the workgroups of a voxel pass, kBoxScanBlock voxels each: <= 2^22, three levels at the most
    uint64_t bytes;                    // of scratch in all
};

// n: the extents of the box.  false: an extent <= 0, or more than kSplitMaxVoxels voxels.
inline bool split_plan(const int32_t n[3], SplitPlan& p) {
    uint64_t voxels = 1;
    for (int a = 0; a < 3; ++a) {
        if (n[a] <= 0) return false;
        if (voxels * (uint64_t)n[a] > kSplitMaxVoxels) return false;      // voxels <= 2^30 and n < 2^31: no overflow
        voxels *= (uint64_t)n[a];
        p.n[a] = (uint32_t)n[a];
    }
    p.voxels = (uint32_t)voxels;
    p.up_off = 0;
    p.uf_off = voxels * 4u;
    p.aux_off = voxels * 8u;
    p.bytes = box_scan_plan((p.voxels + kBoxScanBlock - 1u) / kBoxScanBlock, 4u, voxels * 12u, p.scan);
    return true;
}
