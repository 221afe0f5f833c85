"""Which macro cells a scatter makes stale (csrc/cell_range.h: the cell ranges and launch sizes of the two refresh
passes behind every scatter), and the numpy restatement of the two tables (testing.macro_cells_of) that the GPU tests
hold the device to.  The header is plain C++; it is compiled here on its own with the host compiler.  The driver reads
boxes from stdin and prints the ranges, with the block range's indices folded by the kernels' own cell_torus; the tests
hold them to cells marked in numpy arrays (which cells a box of slots intersects, which cells' 2 x 2 x 2 block holds one
of those), not to a second copy of the arithmetic.  The restatement is held to answers worked out by hand."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from sub_volume_renderer_amd.testing import macro_cells_of

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")

# per line "ox oy oz  nx ny nz  cdx cdy cdz  cshift" -> "raw_c0[3] raw_cn[3] blk_c0[3] blk_cn[3] raw_total blk_total
# raw_blocks blk_blocks" and then, per axis, the blk_cn indices of the block range as the kernels fold them
DRIVER = r"""
#include <stdio.h>
#include "cell_range.h"
int main() {
    for (;;) {
        int32_t off[3], shape[3], cdim[3]; int cshift;
        if (scanf("%d %d %d %d %d %d %d %d %d %d", &off[0], &off[1], &off[2], &shape[0], &shape[1], &shape[2],
                  &cdim[0], &cdim[1], &cdim[2], &cshift) != 10) return 0;
        const CellRanges r = cell_ranges_of(off, shape, cdim, cshift);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u", r.raw_c0[0], r.raw_c0[1], r.raw_c0[2], r.raw_cn[0], r.raw_cn[1],
               r.raw_cn[2], r.blk_c0[0], r.blk_c0[1], r.blk_c0[2], r.blk_cn[0], r.blk_cn[1], r.blk_cn[2], r.raw_total, r.blk_total,
               r.raw_blocks, r.blk_blocks);
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < r.blk_cn[a]; ++k) printf(" %d", cell_torus(r.blk_c0[a] + k, cdim[a]));
        printf("\n");
    }
}
"""

# ring extents in slots (x, y, z) and cshift: 1 to 6 cells on an axis, no two axes of a larger ring alike
RINGS = [((8, 8, 8), 3), ((16, 8, 24), 3), ((24, 16, 40), 3), ((8, 8, 8), 2), ((16, 24, 8), 2)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("cell_range")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def ranges(driver, ring, cshift, boxes):
    """boxes: [(off xyz, shape xyz)] -> per box a dict of the driver's line"""
    cdim = tuple(r >> cshift for r in ring)
    text = "".join("%d %d %d %d %d %d %d %d %d %d\n" % (*off, *shape, *cdim, cshift) for off, shape in boxes)
    lines = [ln for ln in subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split("\n") if ln]
    assert len(lines) == len(boxes)
    out = []
    for ln in lines:
        v = [int(x) for x in ln.split()]
        r = dict(raw_c0=v[0:3], raw_cn=v[3:6], blk_c0=v[6:9], blk_cn=v[9:12], raw_total=v[12], blk_total=v[13], raw_blocks=v[14],
                 blk_blocks=v[15])
        assert len(v) == 16 + sum(r["blk_cn"])
        at = 16
        r["blk_idx"] = []
        for a in range(3):
            r["blk_idx"].append(v[at:at + r["blk_cn"][a]])
            at += r["blk_cn"][a]
        out.append(r)
    return out


def check(ring, cshift, off, shape, r):
    """Every property of the ranges of one box, against cells marked in arrays shaped [z][y][x]."""
    s = 1 << cshift
    cdim = tuple(v >> cshift for v in ring)                           # (x, y, z)
    what = (ring, cshift, off, shape, r)
    slots = np.zeros(ring[::-1], bool)
    slots[off[2]:off[2] + shape[2], off[1]:off[1] + shape[1], off[0]:off[0] + shape[0]] = True
    touched = slots.reshape(cdim[2], s, cdim[1], s, cdim[0], s).any(axis=(1, 3, 5))        # the cells the box intersects
    # the raw range: exactly those, each once, without wrapping
    raw_idx = [list(range(r["raw_c0"][a], r["raw_c0"][a] + r["raw_cn"][a])) for a in range(3)]
    assert all(0 <= i < cdim[a] for a in range(3) for i in raw_idx[a]), what
    cover = np.zeros(touched.shape, int)
    np.add.at(cover, np.ix_(raw_idx[2], raw_idx[1], raw_idx[0]), 1)
    np.testing.assert_array_equal(cover, touched.astype(int), err_msg=f"raw range {what}")
    # the block range: every cell whose 2 x 2 x 2 block (on the torus) holds a refreshed cell
    need = np.zeros_like(touched)
    for d in itertools.product((0, 1), repeat=3):
        need |= np.roll(touched, tuple(-v for v in d), axis=(0, 1, 2))
    for a in range(3):
        idx = r["blk_idx"][a]
        assert all(0 <= i < cdim[a] for i in idx), what
        assert len(set(idx)) == len(idx), f"a cell twice on axis {a}: {what}"
        if r["blk_cn"][a] == cdim[a]:
            assert sorted(idx) == list(range(cdim[a])), what
    count = np.zeros(touched.shape, int)
    np.add.at(count, np.ix_(r["blk_idx"][2], r["blk_idx"][1], r["blk_idx"][0]), 1)
    assert np.all(count[need] >= 1), f"a block that holds a refreshed cell is not refreshed: {what}"
    assert count.max() <= 1, what
    # totals and launch sizes
    assert r["raw_total"] == int(np.prod(r["raw_cn"])) == int(touched.sum()), what
    assert r["blk_total"] == int(np.prod(r["blk_cn"])) == int(count.sum()), what
    assert r["raw_blocks"] == -(-r["raw_total"] // 256) and r["blk_blocks"] == -(-r["blk_total"] // 256), what


@pytest.mark.parametrize("ring,cshift", RINGS, ids=lambda v: str(v))
def test_every_one_axis_box(driver, ring, cshift):
    """Every (offset, length) on one axis, the other two axes pinned to each of three boxes (one voxel at slot 0, one at the
    last slot, the whole axis): the ranges of an axis, exhaustively."""
    boxes = []
    for a in range(3):
        for others in ("first", "last", "all"):
            for o in range(ring[a]):
                for n in range(1, ring[a] - o + 1):
                    off = [0 if others != "last" else ring[b] - 1 for b in range(3)]
                    shape = [ring[b] if others == "all" else 1 for b in range(3)]
                    off[a], shape[a] = o, n
                    boxes.append((tuple(off), tuple(shape)))
    for (off, shape), r in zip(boxes, ranges(driver, ring, cshift, boxes)):
        check(ring, cshift, off, shape, r)


def axis_representatives(n, cshift):
    """Per axis of n slots: for every (first cell, last cell) a box can have, its widest and its narrowest (offset, length),
    plus the two with one end on a cell border and the other off it."""
    s = 1 << cshift
    out = set()
    for c0 in range(n >> cshift):
        for c1 in range(c0, n >> cshift):
            lo_w, lo_n, hi_w, hi_n = c0 * s, c0 * s + s - 1, c1 * s + s, c1 * s + 1        # [lo, hi) with hi exclusive
            for lo, hi in ((lo_w, hi_w), (lo_n, hi_n), (lo_w, hi_n), (lo_n, hi_w)):
                if hi > lo:
                    out.add((lo, hi - lo))
    return sorted(out)


@pytest.mark.parametrize("ring,cshift", RINGS, ids=lambda v: str(v))
def test_boxes_in_three_dimensions(driver, ring, cshift):
    """Every combination of the per-axis representatives as one 3-D box (the rings' axes differ in their number of cells,
    so a range computed from another axis's numbers shows)."""
    reps = [axis_representatives(ring[a], cshift) for a in range(3)]
    boxes = [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for x in reps[0] for y in reps[1] for z in reps[2]]
    if len(boxes) > 4000:                                             # the largest ring: every 7th, still every pair of axes' edges
        boxes = boxes[::7]
    assert len(boxes) >= 8
    for (off, shape), r in zip(boxes, ranges(driver, ring, cshift, boxes)):
        check(ring, cshift, off, shape, r)


@pytest.mark.parametrize("ring,cshift", RINGS, ids=lambda v: str(v))
def test_hand_derived_ranges(driver, ring, cshift):
    cdim = [v >> cshift for v in ring]
    last = tuple(v - 1 for v in ring)
    first_voxel, last_voxel, whole = ranges(driver, ring, cshift, [((0, 0, 0), (1, 1, 1)), (last, (1, 1, 1)), ((0, 0, 0), ring)])
    for a in range(3):
        # a write at slot 0 changes raw cell 0: the blocks that hold it start at cells cdim - 1 (across the seam) and 0
        assert first_voxel["raw_c0"][a] == 0 and first_voxel["raw_cn"][a] == 1
        assert set(first_voxel["blk_idx"][a]) == {cdim[a] - 1, 0} and len(first_voxel["blk_idx"][a]) == min(2, cdim[a])
        # the last slot lies in raw cell cdim - 1: blocks starting at cdim - 2 (folded: cdim 1 -> 0, cdim 2 -> 0) and cdim - 1
        assert last_voxel["raw_c0"][a] == cdim[a] - 1 and last_voxel["raw_cn"][a] == 1
        assert set(last_voxel["blk_idx"][a]) == {(cdim[a] - 2) % cdim[a], cdim[a] - 1} and len(last_voxel["blk_idx"][a]) == min(2, cdim[a])
        # the whole ring: every cell once in both passes
        assert whole["raw_c0"][a] == 0 and whole["raw_cn"][a] == cdim[a]
        assert sorted(whole["blk_idx"][a]) == list(range(cdim[a]))
    n = cdim[0] * cdim[1] * cdim[2]
    assert whole["raw_total"] == whole["blk_total"] == n and whole["raw_blocks"] == whole["blk_blocks"] == -(-n // 256)


# ---- the restatement of the tables, against answers that do not come from it --------------------------------------
def test_restatement_one_bright_voxel_at_slot_0():
    ring = np.zeros((8, 8, 16), np.uint8)                             # [z][y][x]: cdim (x, y, z) = (2, 1, 1) at cshift 3
    ring[0, 0, 0] = 200
    raw, blk = macro_cells_of(ring, 3)
    assert raw.dtype == blk.dtype == np.uint8 and raw.shape == blk.shape == (1, 1, 2)
    assert raw.tolist() == [[[200, 0]]]                               # one cell
    assert blk.tolist() == [[[200, 200]]]                             # cell 1's block wraps to cell 0: both
    raw, blk = macro_cells_of(ring, 2)                                # 4^3 cells: cdim (4, 2, 2); the blocks that hold cell (0,0,0)
    want_raw = np.zeros((2, 2, 4), np.uint8)                          # start at x in {3, 0}, y in {1, 0}, z in {1, 0}
    want_raw[0, 0, 0] = 200
    want_blk = np.zeros((2, 2, 4), np.uint8)
    want_blk[:, :, [0, 3]] = 200
    np.testing.assert_array_equal(raw, want_raw)
    np.testing.assert_array_equal(blk, want_blk)


def test_restatement_floats_nan_infinities_and_wide_integers():
    ring = np.zeros((8, 8, 32), np.float32)                           # four cells along x
    ring[1, 2, 3], ring[7, 7, 7], ring[0, 0, 1] = -3.0, np.nan, 2.0    # cell 0: |-3| wins, the NaN never
    ring[:, :, 8:16] = np.nan                                         # cell 1: nothing but NaN -> 0
    ring[4, 4, 20] = -np.inf                                          # cell 2: |-inf| = +inf
    ring[0, 0, 31] = -0.0                                             # cell 3: |-0| = +0
    raw, blk = macro_cells_of(ring, 3)
    assert raw.dtype == blk.dtype == np.float32
    assert raw.tolist() == [[[3.0, 0.0, np.inf, 0.0]]]
    assert not np.signbit(raw).any()
    assert blk.tolist() == [[[3.0, np.inf, np.inf, 3.0]]]             # blk[x] = max(raw[x], raw[(x + 1) % 4])
    ring = np.zeros((8, 8, 8), np.uint16)
    ring[7, 7, 7], ring[0, 0, 0] = 40000, 39999                       # above 32767: no signed compare
    raw, blk = macro_cells_of(ring, 3)
    assert raw.dtype == np.uint16 and raw.tolist() == [[[40000]]] and blk.tolist() == [[[40000]]]
    ring = np.zeros((8, 8, 8), np.uint8)
    ring[3, 3, 3], ring[3, 3, 4] = 127, 129                           # above 127
    assert macro_cells_of(ring, 3)[0].tolist() == [[[129]]]
