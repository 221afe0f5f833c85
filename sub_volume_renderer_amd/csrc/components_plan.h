// The host plan of svr_components (include/svr.h; kernels: components_kernels.hip): how the voxels of a box are indexed,
// how the context's scratch memory is laid out and how many levels the prefix scan over the roots has.
//
// Plain C++ on plain integers, so that a test can compile it without HIP (tests/test_components.py): svr_components sizes
// the scratch from this plan and svr_launch_components takes extents, counts, scan levels and offsets from it, and
// nowhere else.  The few functions the kernels share with that test are marked COMP_FN.
//
// Layout.  Voxel (rx, ry, rz) of a box of n voxels per axis has the dense index i = (rz n_y + ry) n_x + rx < 2^30.
//   parent  one u32 per voxel: the union-find (components_uf.h); after the flatten pass the root of every inside voxel.
//   aux     one u32 per voxel.  Until the merge pass has run: the label of an inside voxel (what connect() compares).
//           From the rank pass on: at a root, the rank of its component (its number minus one).
//   scan    level 0 holds one u32 per block of kBoxScanBlock voxels, the roots among them; the levels above it are
//           those of box_scan.h.
// The init pass reads a row in the units of box_units.h, 4 ring slots at a multiple of 4: voxel rx of a row is element
// rx + head of it, head (0 .. 3; box_head) being the ring slot of the box's first voxel modulo 4, and a row has upr
// units.  The voxels of one unit are linked along x by the init pass itself (comp_x_implied).
// 8 bytes per voxel, and 4 bytes per 256 voxels for the scan.
#pragma once

#include <stdint.h>

#include "box_scan.h"
#include "box_units.h"

#ifdef __HIPCC__
#define COMP_FN __host__ __device__ __forceinline__
#else
#define COMP_FN inline
#endif

constexpr uint32_t kCompScanBlock = 256;          // voxels per workgroup of the voxel passes: the name tests/test_gpu_components.py sizes its boxes by
static_assert(kCompScanBlock == kBoxScanBlock, "a voxel pass fills one entry of level 0 of the scan per workgroup");
constexpr uint64_t kCompMaxVoxels = 1ull << 30;   // SVR_COMPONENTS_MAX_VOXELS

struct CompPlan {
    uint32_t n[3];                     // voxels per axis (x, y, z)
    uint32_t voxels;                   // n[0] * n[1] * n[2] <= 2^30: every index, and kUfOutside beside them, fits u32
    uint32_t head;                     // elements before a row's first voxel, 0 .. 3
    uint32_t upr;                      // units of 4 ring slots per row
    uint32_t units;                    // upr * n[1] * n[2] <= voxels
    uint64_t parent_off, aux_off;      // byte offsets into the scratch
    BoxScanPlan scan;                  // count[0] = the workgroups of a voxel pass, kBoxScanBlock voxels each: <= 2^22, three levels at the most
    uint64_t bytes;                    // of scratch in all
};

// voxels rx - 1 and rx of a row (rx >= 1) lie in one unit: where they connect, the init pass has linked them already
COMP_FN bool comp_x_implied(uint32_t rx, uint32_t head) { return ((rx + head) & 3u) != 0u; }

// n: the extent of the box, box and window already intersected; head: box_head of its first voxel.  false: the box is
// empty (an n <= 0) or has more than kCompMaxVoxels voxels (*too_many says which).
inline bool comp_plan(const int64_t n[3], uint32_t head, CompPlan& p, bool* too_many = nullptr) {
    if (too_many) *too_many = false;
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) return false;
    uint64_t voxels = 1;
    for (int a = 0; a < 3; ++a) {
        if ((uint64_t)n[a] > kCompMaxVoxels || voxels * (uint64_t)n[a] > kCompMaxVoxels) { if (too_many) *too_many = true; return false; }
        voxels *= (uint64_t)n[a];
        p.n[a] = (uint32_t)n[a];
    }
    p.voxels = (uint32_t)voxels;
    p.head = head;
    p.upr = (p.n[0] + head + 3u) / 4u;
    p.units = p.upr * p.n[1] * p.n[2];           // upr <= n[0] but for rows of one voxel, where it is 1 too
    p.parent_off = 0;
    p.aux_off = voxels * 4u;
    p.bytes = box_scan_plan((p.voxels + kBoxScanBlock - 1u) / kBoxScanBlock, 4u, voxels * 8u, p.scan);
    return true;
}
