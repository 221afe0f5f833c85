"""The march's separable address into the micro-block copy of a ring (csrc/twin_address.h: svr_twin_offset, and the
predicate svr_twin_separable that routes a ring to it).  The header is plain C++; it is compiled here on its own with
the host compiler, and its offsets are held to the layout's definition, restated below: 128-byte blocks in
[bz][by][bx] order, the slots of a block in [z][y][x] order."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")

# offsets <esh> <Rx> <Ry> <Rz> <kx> <ky> <kz> <ox> <oy> <oz>: the byte offset of every voxel of [o, o + ring), x fastest, for
# a lane whose ring slot is voxel + k, as raw uint32 on stdout;  pred <esh> <Rx> <Ry>: "<0|1> <Wy> <Wz>"
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "twin_address.h"
template <int ESH> static int sweep(char** a) {
    typedef TwinBlock<ESH> B;
    const uint32_t R[3] = { (uint32_t)atoi(a[0]), (uint32_t)atoi(a[1]), (uint32_t)atoi(a[2]) };
    const int k[3] = { atoi(a[3]), atoi(a[4]), atoi(a[5]) };
    const uint32_t o[3] = { (uint32_t)atoi(a[6]), (uint32_t)atoi(a[7]), (uint32_t)atoi(a[8]) };
    const uint32_t w = svr_twin_weights(ESH, R[0], R[1]);
    if (!w) return 2;
    const uint32_t Kb = (uint32_t)((k[2] >> B::ZB) * (int)(R[1] >> B::YB) + (k[1] >> B::YB)) * (R[0] >> B::XB) + (uint32_t)(k[0] >> B::XB);
    const uint32_t Kp = svr_twin_lane_const<ESH>(Kb);
    std::vector<uint32_t> out;
    for (uint32_t z = o[2]; z < o[2] + R[2]; ++z)
        for (uint32_t y = o[1]; y < o[1] + R[1]; ++y)
            for (uint32_t x = o[0]; x < o[0] + R[0]; ++x)
                out.push_back(svr_twin_offset<ESH>(x, y | z << 16, w, Kp));
    return fwrite(out.data(), 4, out.size(), stdout) == out.size() ? 0 : 1;
}
int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "pred")) {
        const int esh = atoi(argv[2]);
        const uint32_t Rx = (uint32_t)atoi(argv[3]), Ry = (uint32_t)atoi(argv[4]);
        printf("%d %llu %llu\n", svr_twin_separable(esh, Rx, Ry) ? 1 : 0, (unsigned long long)svr_twin_wy(esh, Rx),
               (unsigned long long)svr_twin_wz(esh, Rx, Ry));
        return 0;
    }
    if (argc != 12 || strcmp(argv[1], "offsets")) return 3;
    const int esh = atoi(argv[2]);
    return esh == 0 ? sweep<0>(argv + 3) : (esh == 1 ? sweep<1>(argv + 3) : sweep<2>(argv + 3));
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("twin_address")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def layout_offsets(esh, ring, k=(0, 0, 0), origin=(0, 0, 0)):
    """The definition: byte offset, mod 2^32, of the slots voxel + k of the voxels [origin, origin + ring) (z, y, x order,
    x fastest) in the micro-block copy.  Slots outside the ring continue the same index linearly (floor shifts, the
    block number taken as it comes): what the march's address arithmetic, all of it mod 2^32, means by a lane's
    constants before they have brought the slot into the ring."""
    rx, ry, rz = ring
    xb, yb, zb = (3 if esh == 0 else 2), 2, (1 if esh == 2 else 2)
    z, y, x = np.meshgrid(*(np.arange(origin[a] + k[a], origin[a] + k[a] + ring[a], dtype=np.int64) for a in (2, 1, 0)), indexing="ij")
    block = ((z >> zb) * (ry >> yb) + (y >> yb)) * (rx >> xb) + (x >> xb)                      # [bz][by][bx]
    inside = (((z & ((1 << zb) - 1)) << yb | (y & 3)) << xb) | (x & ((1 << xb) - 1))           # [z][y][x]
    element = (block << (7 - esh)) + inside
    return ((element << esh) & 0xFFFFFFFF).ravel()


def test_the_restated_layout_is_a_permutation_of_the_ring_in_whole_blocks():
    for esh, ring in ((0, (24, 20, 8)), (1, (64, 24, 8)), (2, (40, 36, 4))):
        off = layout_offsets(esh, ring)
        assert np.array_equal(np.sort(off), np.arange(ring[0] * ring[1] * ring[2]) << esh)
        first = off.reshape(ring[2], ring[1], ring[0])[:(2 if esh == 2 else 4), :4, :(8 if esh == 0 else 4)]
        assert np.array_equal(first.ravel(), np.arange(128 >> esh) << esh)                     # block 0: slots in [z][y][x] order


@pytest.mark.parametrize("ring", [(24, 20, 8), (64, 24, 8), (40, 36, 4)], ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("esh", [0, 1, 2], ids=["uint8", "uint16", "float32"])
def test_every_slot_of_small_rings_under_every_wrap_constant(driver, esh, ring):
    """Exhaustive: the voxels [0, ring) under wrap constants of 0, +ring and -ring on each axis (27 combinations) against
    the definition at voxel + k; and, for the constants the march really carries (none positive), the voxels
    [-k, ring - k) whose slots are the ring itself."""
    def offsets(k, origin):
        raw = subprocess.run([driver, "offsets", str(esh), *map(str, ring), *map(str, k), *map(str, origin)], check=True,
                             capture_output=True).stdout
        return np.frombuffer(raw, dtype=np.uint32)

    in_ring = layout_offsets(esh, ring)
    for kz in (0, ring[2], -ring[2]):
        for ky in (0, ring[1], -ring[1]):
            for kx in (0, ring[0], -ring[0]):
                k = (kx, ky, kz)
                cases = [((0, 0, 0), layout_offsets(esh, ring, k))]
                if max(k) <= 0:
                    cases.append((tuple(-v for v in k), in_ring))
                for origin, want in cases:
                    got = offsets(k, origin)
                    assert got.size == want.size
                    bad = np.flatnonzero(got != want)
                    assert bad.size == 0, (esh, ring, k, origin, bad[:5], got[bad[:5]], want[bad[:5]])


def test_predicate_at_its_edge(driver):
    def ask(esh, rx, ry):
        ok, wy, wz = subprocess.run([driver, "pred", str(esh), str(rx), str(ry)], check=True, capture_output=True, text=True).stdout.split()
        return ok == "1", int(wy), int(wz)

    assert ask(0, 1024, 512) == (True, 511, 65532)
    assert ask(0, 1024, 516)[0] is False and ask(0, 1024, 516)[2] > 65535
    assert ask(0, 528, 512) == (True, 263, 4 * (66 * 128 - 1))                 # the benchmark's finest ring plane
    assert ask(0, 2048, 2048)[0] is False                                       # a 2048^3-class finest ring
    # two- and four-byte elements: blocks of 4 x 4 x 4 and 4 x 4 x 2, weights in units of 32 resp. 64 bytes
    assert ask(1, 512, 512) == (True, 511, 65532) and ask(1, 512, 516)[0] is False
    assert ask(2, 1024, 512) == (True, 511, 65534) and ask(2, 1024, 516)[0] is False
    for esh in (0, 1, 2):
        assert ask(esh, 24, 20)[0] and ask(esh, 8, 4)[0]
