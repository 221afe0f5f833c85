// Which macro cells a scatter box makes stale: the cell ranges and grid sizes of the two refresh passes of
// svr_launch_cell_update (ring_kernels.hip).  Plain host C++ on plain integers, so that a test can compile it without
// HIP (tests/test_cell_range.py).
#pragma once

#include <stdint.h>

struct CellRanges {
    int32_t raw_c0[3], raw_cn[3];      // cells whose slots the box touches: [raw_c0, raw_c0 + raw_cn), inside the grid
    int32_t blk_c0[3], blk_cn[3];      // cells whose 2 x 2 x 2 block holds one of those; blk_c0 may be -1: the kernels
                                       // wrap every index of a range on the torus
    int32_t raw_total, blk_total;      // threads of the two passes
    uint32_t raw_blocks, blk_blocks;   // workgroups of 256
};

// off, shape: the box in ring slots (shape > 0 on every axis, off + shape <= the ring's extent); cdim: cells per axis.
static inline CellRanges cell_ranges_of(const int32_t off[3], const int32_t shape[3], const int32_t cdim[3], int cshift) {
    CellRanges r;
    for (int i = 0; i < 3; ++i) {
        r.raw_c0[i] = off[i] >> cshift;
        r.raw_cn[i] = ((off[i] + shape[i] - 1) >> cshift) - r.raw_c0[i] + 1;
        // the blocks that contain a refreshed cell start one cell earlier; a range as long as the axis is the whole axis
        r.blk_c0[i] = r.raw_c0[i] - 1;
        r.blk_cn[i] = r.raw_cn[i] + 1 > cdim[i] ? cdim[i] : r.raw_cn[i] + 1;
    }
    r.raw_total = r.raw_cn[0] * r.raw_cn[1] * r.raw_cn[2];
    r.blk_total = r.blk_cn[0] * r.blk_cn[1] * r.blk_cn[2];
    r.raw_blocks = (unsigned)((r.raw_total + 255) / 256);
    r.blk_blocks = (unsigned)((r.blk_total + 255) / 256);
    return r;
}

// how the kernels fold an index of a range back into [0, n) (the one function of this header that device code calls)
#ifdef __HIPCC__
__host__ __device__ __forceinline__
#else
static inline
#endif
int cell_torus(int c, int n) { c %= n; return c < 0 ? c + n : c; }
