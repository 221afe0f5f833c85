// The host plan of svr_mesh (include/svr.h; kernels: mesh_kernels.hip): how the voxels and cells of a box are laid out
// in the context's scratch memory and how many levels the prefix scan over the cells has.
//
// Plain C++ on plain integers, so that a test can compile it without HIP (tests/test_mesh.py): svr_mesh sizes the
// scratch from this plan and svr_launch_mesh takes extents, word counts, scan levels and offsets from it, and nowhere else.
//
// Layout.  A box of n voxels per axis has n + 1 cells per axis.
//   bits   one bit per voxel, inside or not: a row of voxels (along x) is `bpr` u32 words, voxel r of the row is bit
//          r + head of it.  head (0 .. 3; box_units.h: box_head) is the ring slot of the box's first voxel modulo 4, so
//          that a group of 4 bits at a multiple of 4 is 4 ring slots at a multiple of 4: one unit of box_units.h, an
//          aligned 16-byte load of a 4-byte ring.  The bits below head and beyond the row are zero.
//   cells  4 bits per cell (bit 0 / 1 / 2: the lattice edge that leaves the cell's first corner along x / y / z crosses
//          the surface; bit 3: the cell is active); 16 cells are one 64-bit word, and a row of cells is a whole number
//          of words, so that a word never spans two rows; the cells a row's last word has too many are zero.  Words are
//          in row order (z, then y), which is the order of vertices and quads.
//   scan   level 0 holds two u32 counts per word of cells (active cells, crossing edges); the levels above it are those
//          of box_scan.h.
// About 1 byte per cell for cells and scan, and an eighth of a byte per voxel for the bits.
#pragma once

#include <stdint.h>

#include "box_scan.h"
#include "box_units.h"

constexpr uint32_t kMeshCellsPerWord = 16;
constexpr uint32_t kMeshScanBlock = 256;          // words of cells per scan block: the name tests/test_gpu_mesh.py sizes its windows by
static_assert(kMeshScanBlock == kBoxScanBlock, "the scan of box_scan.h is the one that runs");
constexpr uint64_t kMeshMaxCells = 1ull << 28;    // SVR_MESH_MAX_CELLS

struct MeshPlan {
    uint32_t n[3];                     // voxels per axis (x, y, z)
    uint32_t cells[3];                 // n + 1
    uint32_t head;                     // bits before a row's first voxel, 0 .. 3
    uint32_t bpr;                      // u32 words of bits per row of voxels
    uint32_t bit_words;                // bpr * n[1] * n[2]
    uint32_t wpr;                      // words per row of cells
    uint32_t rows;                     // cells[1] * cells[2]
    uint32_t words;                    // wpr * rows  (<= the number of cells)
    uint64_t nib_off;                  // byte offsets into the scratch: the words of cells,
    BoxScanPlan scan;                  // the scan (8 bytes per entry; count[0] = words <= 2^28: four levels at the most),
    uint64_t bit_off;                  // the bits
    uint64_t bytes;                    // of scratch in all
};

// n: the extent of the box, box and window already intersected; head: box_head of its first voxel.  false: the box is
// empty (an n <= 0) or has more than kMeshMaxCells cells (*too_many says which).
inline bool mesh_plan(const int64_t n[3], uint32_t head, MeshPlan& p, bool* too_many = nullptr) {
    if (too_many) *too_many = false;
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) return false;
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        const uint64_t c = (uint64_t)n[a] + 1u;
        if (c > kMeshMaxCells || cells * c > kMeshMaxCells) { if (too_many) *too_many = true; return false; }
        cells *= c;
        p.n[a] = (uint32_t)n[a];
        p.cells[a] = (uint32_t)c;
    }
    p.head = head;
    p.bpr = (p.n[0] + head + 31u) / 32u;
    p.bit_words = p.bpr * p.n[1] * p.n[2];       // bpr <= n[0]: fewer words than voxels
    p.wpr = (p.cells[0] + kMeshCellsPerWord - 1u) / kMeshCellsPerWord;
    p.rows = p.cells[1] * p.cells[2];
    p.words = p.wpr * p.rows;                    // wpr <= cells[0]: no more words than cells
    p.nib_off = 0;
    uint64_t at = box_scan_plan(p.words, 8u, (uint64_t)p.words * 8u, p.scan);
    p.bit_off = at;
    at += (uint64_t)p.bit_words * 4u;
    p.bytes = at;
    return true;
}
