"""The plan of a streaming pass over a box of one LOD's window (csrc/ring_pieces.h): the cut at the ring's wrap seams
into at most 2 x 2 x 2 dense pieces, the rows a workgroup takes, the 16-byte slots of a row and the lanes that share it.
The header's host half is plain C++; it is compiled here on its own with the host compiler.  The driver reads cases from
stdin and prints the plan; the tests hold it to properties worked out here with numpy and plain Python (marking the
pieces in a ring-shaped array, the row starts of the ring one by one), not to a second copy of the planner."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from odd_ring_scenes import plan_cases

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")

# per line "rx ry rz  ox oy oz  lox loy loz  nx ny nz  bytes_per_voxel per_slot slot_base workgroups min_share" ->
# "blocks npieces" and per piece "s[3] n[3] rel[3] rows rows_per_wg block0 lpr_log2 spr", or "fail"
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include "ring_pieces.h"
int main() {
    for (;;) {
        uint32_t ring[3]; int32_t off[3]; int64_t lo[3], n[3]; RingPass pass;
        if (scanf("%" SCNu32 "%" SCNu32 "%" SCNu32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNd64
                  "%" SCNu32 "%" SCNu32 "%" SCNu64 "%" SCNu64 "%" SCNu64,
                  &ring[0], &ring[1], &ring[2], &off[0], &off[1], &off[2], &lo[0], &lo[1], &lo[2], &n[0], &n[1], &n[2],
                  &pass.bytes_per_voxel, &pass.per_slot, &pass.slot_base, &pass.workgroups, &pass.min_share) != 17) return 0;
        RingPlan plan;
        if (!ring_plan(ring, off, lo, n, pass, plan)) { printf("fail\n"); continue; }
        printf("%" PRIu32 " %d", plan.blocks, (int)plan.pieces.npieces);
        for (int p = 0; p < plan.pieces.npieces; ++p) {
            const RingPiece& P = plan.pieces.piece[p];
            printf(" %u %u %u %u %u %u %u %u %u %u %u %u %u %u", P.s[0], P.s[1], P.s[2], P.n[0], P.n[1], P.n[2], plan.rel[p][0],
                   plan.rel[p][1], plan.rel[p][2], P.rows, P.rows_per_wg, P.block0, P.lpr_log2, P.spr);
        }
        printf("\n");
    }
}
"""

# (bytes read per voxel, voxels per 16-byte slot): the histogram on u8 / u16 / f32 rings, the objects pass on each
HIST = {1: (1, 16), 2: (2, 8), 4: (4, 4)}
OBJ = {1: (5, 4), 2: (6, 4), 4: (8, 4)}
ALIGNED, NO_POINTER = 0x7F0000001000, 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("ring_pieces")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def case(ring, lo, n, consts, base=ALIGNED, off=None, workgroups=2048, min_share=16384):
    return dict(ring=tuple(ring), off=tuple(lo) if off is None else tuple(off), lo=tuple(lo), n=tuple(n), bpv=consts[0], per_slot=consts[1],
                base=base, workgroups=workgroups, min_share=min_share)


def plans(driver, cases):
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (*c["ring"], *c["off"], *c["lo"], *c["n"], c["bpv"], c["per_slot"],
                                                                         c["base"], c["workgroups"], c["min_share"]) for c in cases)
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    lines = [ln for ln in lines if ln]
    assert len(lines) == len(cases)
    out = []
    for ln in lines:
        assert ln != "fail"
        v = [int(x) for x in ln.split()]
        assert len(v) == 2 + 14 * v[1]
        pieces = []
        for p in range(v[1]):
            w = v[2 + 14 * p: 16 + 14 * p]
            pieces.append(dict(s=w[0:3], n=w[3:6], rel=w[6:9], rows=w[9], rows_per_wg=w[10], block0=w[11], lpr_log2=w[12], spr=w[13]))
        out.append((v[0], pieces))
    return out


def check(c, plan, mark=True):
    """Every property of one plan.  -> its pieces."""
    blocks, pieces = plan
    ring, lo, n, off, ps = c["ring"], c["lo"], c["n"], c["off"], c["per_slot"]
    es = 16 // ps
    assert 1 <= len(pieces) <= 8
    if mark:
        # the pieces' slots, marked in a ring-shaped array (numpy order z, y, x), against (lo + i) mod ring for i < n
        got = np.zeros(ring[::-1], np.int32)
        for P in pieces:
            s, m = P["s"], P["n"]
            got[s[2]:s[2] + m[2], s[1]:s[1] + m[1], s[0]:s[0] + m[0]] += 1
        want = np.zeros(ring[::-1], np.int32)
        want[np.ix_(*[(lo[a] + np.arange(n[a])) % ring[a] for a in (2, 1, 0)])] = 1
        assert np.array_equal(got, want), (c, pieces)
    else:
        # too large to mark: the same per axis, and the pieces are the product of the axes' runs
        runs = [sorted({(P["s"][a], P["n"][a]) for P in pieces}) for a in range(3)]
        for a in range(3):
            slots = sorted(x for s, m in runs[a] for x in (range(s, s + m) if m < 1000 else (s, s + m - 1)))
            if n[a] < 1000:
                assert slots == sorted((lo[a] + i) % ring[a] for i in range(n[a])), (c, a)
            assert sum(m for _, m in runs[a]) == n[a] and all((s - lo[a]) % ring[a] < n[a] for s, _ in runs[a]), (c, a)
        combos = sorted(tuple((P["s"][a], P["n"][a]) for a in range(3)) for P in pieces)
        assert combos == sorted(itertools.product(*runs)), c
    total = 0
    for P in pieces:
        s, m = P["s"], P["n"]
        for a in range(3):
            assert m[a] >= 1 and s[a] + m[a] <= ring[a], (c, P)
            first = lo[a] + (s[a] - lo[a]) % ring[a]           # the logical coordinate in the box that sits in slot s
            assert lo[a] <= first < lo[a] + n[a] and P["rel"][a] == first - off[a], (c, P)
        rows, rpw = P["rows"], P["rows_per_wg"]
        assert rows == m[1] * m[2]
        assert 1 <= rpw <= rows and rpw * m[0] < 2 ** 32, (c, P)
        assert P["block0"] == total, (c, P)
        total += -(-rows // rpw)
        # the elements before a row in its first slot: the row starts of the ring, one by one (the starts repeat after
        # at most per_slot rows); the piece's rows are among them
        assert c["base"] % es == 0
        heads = {((c["base"] + (k * ring[0] + s[0]) * es) % 16) // es for k in range(ps)}
        spr = P["spr"]
        assert all(spr * ps >= h + m[0] for h in heads), (c, P)                      # covers every row
        assert (spr - 1) * ps < max(heads) + m[0], (c, P)                              # one slot fewer would not
        lg = P["lpr_log2"]
        assert lg <= 8 and 2 ** lg >= min(spr, 8), (c, P)
        if spr <= 8:
            assert 2 ** lg < 2 * spr, (c, P)                                           # the smallest power of two that covers
        else:
            padded = {g: -(-spr // 2 ** g) * 2 ** g for g in range(3, 9)}
            assert lg == max(g for g in padded if padded[g] == min(padded.values())), (c, P, padded)
    assert total == blocks
    return pieces


def test_seams(driver):
    ring = (48, 40, 36)
    cases, want = [], []
    for k, (lo, n, npieces) in enumerate([
            ((3, 2, 1), (40, 30, 30), 1),                                  # no seam
            ((20, 2, 1), (40, 30, 30), 2), ((3, 20, 1), (40, 30, 30), 2), ((3, 2, 20), (40, 30, 30), 2),     # one seam per axis
            ((20, 20, 20), (40, 30, 30), 8),                               # all three
            ((47, 39, 35), (2, 2, 2), 8),                                  # 8 pieces of one voxel
            ((96, 80, 72), (48, 40, 36), 1), ((0, 0, 0), (48, 40, 36), 1),  # lo a multiple of the ring; the whole ring
            ((48 * 7 + 1, 40 * 3, 36 * 5 + 35), (48, 40, 36), 4),          # a whole ring's worth that starts inside it
            ((-5, -41, -36), (10, 3, 2), 4),                               # negative logical coordinates
            ((17, 23, 31), (1, 1, 1), 1), ((47, 39, 35), (1, 1, 1), 1)]):  # one voxel
        for consts in (HIST[1], HIST[2], HIST[4], OBJ[1]):
            cases.append(case(ring, lo, n, consts, off=(lo[0] - 3, lo[1], lo[2] - k)))
            want.append(npieces)
    for c, plan, npieces in zip(cases, plans(driver, cases), want):
        assert len(check(c, plan)) == npieces, c


def test_slots_and_lanes_per_row(driver):
    cases = []
    for es in (1, 2, 4):
        for consts, bases in ((HIST[es], (ALIGNED, ALIGNED + es, ALIGNED + 16 - es)),
                              (OBJ[es], (ALIGNED, ALIGNED + 4, ALIGNED + 12, NO_POINTER))):
            ps = consts[1]
            # rows shorter than one slot, of exactly 1, 8, 9 and 257 slots and one element either side of each
            lengths = sorted({1, 2, ps - 1} | {v for k in (1, 8, 9, 257) for v in (k * ps - 1, k * ps, k * ps + 1)})
            for ring_x in (4352, 4353, 4360, 4354):                       # pitch of whole slots, odd, and in between
                for base in bases:
                    for n0 in lengths:
                        for s0 in (0, 1, ps - 1, ps, 4352 - n0):
                            cases.append(case((ring_x, 5, 3), (s0, 1, 1), (n0, 3, 2), consts, base=base))
    seen = set()
    for c, plan in zip(cases, plans(driver, cases)):
        (P,) = check(c, plan, mark=False)
        seen.add(P["spr"])
    assert {1, 2, 8, 9, 10, 257, 258} <= seen
    # exactly 8, 9 and 257 slots on aligned rows: 8 lanes, 16 lanes (one pass), 8 lanes (264 slots, 7 wasted)
    for slots, lg in ((8, 3), (9, 4), (257, 3)):
        c = case((4352, 5, 3), (0, 0, 0), (slots * 16, 5, 3), HIST[1])
        (P,) = check(c, plans(driver, [c])[0], mark=False)
        assert (P["spr"], P["lpr_log2"]) == (slots, lg)


def test_shares(driver):
    ring = (528, 512, 512)
    cases = [case(ring, (0, 0, 0), ring, HIST[1]),                                        # 8 workgroups on each of 256 CUs
             case(ring, (16, 500, 500), (500, 100, 100), OBJ[4], workgroups=768, min_share=65536),
             case(ring, (0, 0, 0), ring, HIST[1], workgroups=10 ** 9, min_share=1),         # a share below one row
             case(ring, (100, 100, 100), (7, 9, 11), HIST[2], workgroups=1, min_share=1),
             case(ring, (0, 0, 0), (528, 4, 4), HIST[4], min_share=1 << 40)]               # one workgroup takes all
    got = [check(c, plan, mark=False) for c, plan in zip(cases, plans(driver, cases))]
    assert got[0][0]["rows_per_wg"] == -(-(528 * 512 * 512 // 2048) // 528)
    assert all(P["rows_per_wg"] == 1 for P in got[2]) and got[3][0]["rows_per_wg"] == got[3][0]["rows"] == 99
    assert got[4][0]["rows_per_wg"] == 16 and len(got[1]) == 4
    # the u32 cap: rows of 2^24 - 1 voxels, 400 of them, and a share of all of them: 256 rows would be 2^32 - 256 voxels
    big = case((2 ** 24 + 5, 24, 24), (3, 2, 1), (2 ** 24 - 1, 20, 20), HIST[1], workgroups=1)
    (P,) = check(big, plans(driver, [big])[0], mark=False)
    assert P["rows"] == 400 and P["rows_per_wg"] == (2 ** 32 - 1) // (2 ** 24 - 1) == 256
    wrapped = case((2 ** 24 + 5, 24, 24), (9, 20, 1), (2 ** 24 - 1, 20, 20), OBJ[1], workgroups=1, base=NO_POINTER)
    assert len(check(wrapped, plans(driver, [wrapped])[0], mark=False)) == 4


def test_windows_and_boxes_of_the_odd_ring_scenes(driver):
    """What tests/test_gpu_odd_rings.py asks the plan for: rings of 63, 21, 42, 36, 40, 3 and 1 voxels along x, windows
    of a whole ring's worth that begin inside it, one at 2^31 - 1 - shape, and the boxes of the 63-voxel ring; the
    histogram on each storage and the objects pass, with and without a label ring to align to."""
    cases = []
    for ring, off, lo, n in plan_cases():
        for consts, base in ((HIST[1], ALIGNED), (HIST[2], ALIGNED), (HIST[4], ALIGNED), (OBJ[1], ALIGNED), (OBJ[4], NO_POINTER)):
            cases.append(case(ring, lo, n, consts, base=base, off=off))
    assert len(cases) == 5 * (7 * 5 + 2 + 34)
    spr_by_ring = {}
    for c, plan in zip(cases, plans(driver, cases)):
        pieces = check(c, plan)
        assert len(pieces) == np.prod([1 + (c["lo"][a] % c["ring"][a] + c["n"][a] > c["ring"][a]) for a in range(3)])
        if c["n"] == c["ring"]:
            spr_by_ring.setdefault((c["ring"][0], c["per_slot"]), set()).update(P["spr"] for P in pieces)
    # a row of one voxel takes one slot whatever comes before it; a row of 3 voxels may lie in two slots of 4
    assert spr_by_ring[(1, 4)] == {1} and spr_by_ring[(1, 16)] == {1} and 2 in spr_by_ring[(3, 4)]


def test_every_box_of_a_small_ring(driver):
    ring = (8, 5, 3)
    variants = [dict(consts=HIST[1], base=ALIGNED), dict(consts=HIST[4], base=ALIGNED + 4), dict(consts=OBJ[2], base=NO_POINTER)]
    cases = []
    for k, (lo, n) in enumerate(itertools.product(itertools.product(range(8), range(5), range(3)),
                                                  itertools.product(range(1, 9), range(1, 6), range(1, 4)))):
        v = variants[(sum(lo) + sum(n)) % 3]
        cases.append(case(ring, lo, n, v["consts"], base=v["base"], off=(lo[0] - k % 4, lo[1], lo[2] - k % 2), workgroups=1 + k % 7,
                          min_share=(1, 24, 16384)[(k // 5) % 3]))
    assert len(cases) == 120 * 120
    for c, plan in zip(cases, plans(driver, cases)):
        pieces = check(c, plan)
        assert len(pieces) == np.prod([1 + (c["lo"][a] % ring[a] + c["n"][a] > ring[a]) for a in range(3)])
