"""svr_distance without a GPU: the numpy restatement (tests/distance_twin.py) held to scipy.ndimage.distance_transform_edt
and, for inside(), to tests/components_twin.py; the 1-D scan, the x pass and the host plan (csrc/distance_scan.h,
csrc/distance_plan.h) compiled on their own with the host compiler, address and undefined-behaviour sanitizers on, into
a program of its own that is run directly, and compared with brute force; and the pins of the new surface (the symbol,
the struct sizes, the argument errors of ``SubVolume.distance``, the arithmetic of ``DistanceField``)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from components_twin import components_twin
from distance_twin import FAR, axis_minimum, box_and_inside, count_only, distance_twin, squared_edt
from odd_ring_scenes import plan_cases
from sub_volume_renderer_amd import DistanceField, SubVolume, SubVolumeMaterial, _native as N
from sub_volume_renderer_amd.distance import distance_arguments, signed_squared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
MAX_EXTENT = 16384


def volumes():
    rng = np.random.default_rng(33)
    shape = (9, 11, 14)
    noise = rng.random(shape)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    ball = (x - 6) ** 2 + (y - 5) ** 2 + (z - 4) ** 2 <= 14
    return [("54 %", noise < 0.54), ("97 %", noise < 0.97), ("3 %", noise < 0.03), ("ball", ball), ("checkerboard", (x + y + z) % 2 == 0),
            ("all", np.ones(shape, bool)), ("none", np.zeros(shape, bool)), ("one row", rng.random((1, 1, 37)) < 0.8),
            ("one column", rng.random((23, 1, 1)) < 0.8), ("one voxel", np.ones((1, 1, 1), bool))]


def scipy_squared(inside):
    return np.rint(ndimage.distance_transform_edt(inside) ** 2).astype(np.int64)


# ---- the twin against scipy ----------------------------------------------------------------------------------------------
def test_twin_is_scipy_edt_squared():
    for name, inside in volumes():
        for invert in (False, True):
            target = ~inside if invert else inside
            got = squared_edt(~target, border=False)
            assert got.dtype == np.int32
            if (~target).any():                             # scipy answers only where at least one source exists
                assert np.array_equal(got, scipy_squared(target)), (name, invert)
                assert not (got == FAR).any()
            else:
                assert (got == FAR).all(), (name, invert)
            # border: the array padded by one voxel of outside, cropped back
            got = squared_edt(~target, border=True)
            want = scipy_squared(np.pad(target, 1, constant_values=False))[1:-1, 1:-1, 1:-1]
            assert np.array_equal(got, want), (name, invert, "border")


def test_twin_inside_is_the_components_twins():
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 3, (6, 7, 8)).astype(np.uint32)
    density = rng.random((6, 7, 8)).astype(np.float32)
    density[1, 2, 3] = np.nan
    off = (16, 8, 40)
    for mode in (dict(level=0.6), dict(), dict(ignore_zero=True), dict(selected=[2, 9], ignore_zero=True), dict(selected=[0, 1], ignore_zero=True),
                 dict(level=0.5, box=((10, 10, 42), (9, 3, 100))), dict(box=((0, 0, 0), (5, 5, 5))), dict(box=((17, 9, 41), (0, 2, 2)), level=0.1)):
        for lab in (labels, None):
            comp = components_twin(off, density, lab, join_labels=True, connectivity=26, **mode)
            _, lo, n, inside, dropped = box_and_inside(off, density, lab, **mode)
            twin = distance_twin(off, density, lab, **mode)
            assert twin["header"][4:14] == comp["header"][4:14] and twin["header"][1] == comp["header"][1], mode
            if inside is None:
                assert comp["ids"].size == 0 and twin["header"] == [0, 0, 0, 0, 16, 8, 40] + [0] * 9 and twin["d2"].shape == (0, 0, 0)
            else:
                assert np.array_equal(inside, comp["ids"] != 0) and dropped == comp["header"][13], mode
    assert distance_twin((3, 4, 5), None, None, level=1.0)["header"] == [0, 0, 0, 0, 3, 4, 5] + [0] * 9


def test_twin_header_invert_border_and_far():
    rng = np.random.default_rng(9)
    density = rng.random((6, 7, 8)).astype(np.float32)
    off = (16, 8, 40)
    inside = density >= np.float32(0.3)
    twin = distance_twin(off, density, None, level=0.3)
    want = scipy_squared(inside)
    top = int(want.max())
    assert twin["header"] == [int(inside.sum()), int(inside.sum()), inside.size, top, 16, 8, 40, 16, 8, 40, 8, 7, 6, 0,
                              int(np.flatnonzero(want.reshape(-1) == top)[0]), 0]
    assert np.array_equal(twin["d2"], want)
    inv = distance_twin(off, density, None, level=0.3, invert=True, border=True)              # border is not read
    assert np.array_equal(inv["d2"], scipy_squared(~inside)) and inv["header"][:2] == [int((~inside).sum()), int(inside.sum())]
    plain = distance_twin(off, density, None, level=0.3, invert=True, border=False)
    assert inv["header"] == plain["header"] and np.array_equal(inv["d2"], plain["d2"])
    # no source at all: FAR everywhere without a border, the pure face distance with one
    solid = distance_twin(off, density, None, level=-1.0)
    assert (solid["d2"] == FAR).all() and solid["header"][:4] == [336, 336, 336, 0] and solid["header"][14:] == [0, 336]
    faces = distance_twin(off, density, None, level=-1.0, border=True)
    z, y, x = np.meshgrid(np.arange(6), np.arange(7), np.arange(8), indexing="ij")
    face = np.minimum.reduce([x + 1, 8 - x, y + 1, 7 - y, z + 1, 6 - z])
    assert np.array_equal(faces["d2"], face ** 2) and faces["header"][3] == 9 and faces["header"][15] == 0
    assert faces["header"][14] == (2 * 7 + 2) * 8 + 2                  # the first voxel three deep: (2, 2, 2)
    nothing = distance_twin(off, density, None, level=2.0, invert=True)
    assert (nothing["d2"] == FAR).all() and nothing["header"][:2] == [336, 0] and nothing["header"][15] == 336
    empty = distance_twin(off, density, None, level=2.0, border=True)
    assert not empty["d2"].any() and empty["header"][:4] == [0, 0, 336, 0] and empty["header"][14:] == [0, 0]
    assert count_only(twin["header"]) == twin["header"][:2] + [0, 0] + twin["header"][4:14] + [0, 0]
    # a box partly outside the window is cut at the window
    part = distance_twin(off, density, None, box=((10, 10, 42), (9, 3, 100)), level=0.5, border=True)
    inner = density[2:, 2:5, :3] >= np.float32(0.5)
    assert part["header"][7:13] == [16, 10, 42, 3, 3, 4]
    assert np.array_equal(part["d2"], scipy_squared(np.pad(inner, 1, constant_values=False))[1:-1, 1:-1, 1:-1])


# ---- the scan, the x pass and the plan on the host ----------------------------------------------------------------------------
# "scan IN OUT stride ring": IN holds int32 words: the number of columns, then per column its length m and its m entries; OUT
#   receives every column's result.  A column is scanned in place, strided as the kernel strides it, canaries between.
# "rows": reads "n head bits" lines (bits: a string of 0 and 1, a 1 being a source) -> a line of n squared distances each.
# "plan": reads "nx ny nz head" lines -> "voxels head wpr upr units columns[2] bits_off stack_off bytes", "empty", "extent" or "voxels".
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "distance_plan.h"
#include "distance_scan.h"

static int scan(int argc, char** argv) {
    if (argc != 6) return 2;
    const size_t stride = (size_t)atoi(argv[4]);
    const int ring_size = atoi(argv[5]);
    FILE* f = fopen(argv[2], "rb");
    FILE* o = fopen(argv[3], "wb");
    int32_t count = 0;
    if (!f || !o || fread(&count, 4, 1, f) != 1) return 4;
    for (int32_t k = 0; k < count; ++k) {
        int32_t m = 0;
        if (fread(&m, 4, 1, f) != 1 || m < 1) return 4;
        std::vector<int32_t> in((size_t)m);
        if (fread(in.data(), 4, (size_t)m, f) != (size_t)m) return 4;
        // exactly as long as the last element needs: one step too many is out of bounds
        std::vector<int32_t> g(((size_t)m - 1) * stride + 1, -77);
        std::vector<DistEntry> stack(((size_t)m - 1) * stride + 1, DistEntry{-77, 77u});
        for (int32_t u = 0; u < m; ++u) g[(size_t)u * stride] = in[(size_t)u];
        int32_t* col = g.data();
        uint32_t calls = 0, last = (uint32_t)m;
        bool ordered = true;
        auto emit = [&](uint32_t u, int32_t v) {
            ordered = ordered && u + 1u == last; last = u; ++calls;
            col[(size_t)u * stride] = v;
        };
        // the ring of the last entries pushed: exactly its slots, strided too; 1 and 4 slots, so that most pops miss it
        std::vector<DistEntry> slots(((size_t)ring_size - 1) * stride + 1, DistEntry{-77, 77u});
        if (ring_size == 1) dist_scan_column(col, stride, (uint32_t)m, stack.data(), stride, DistRing<1>(slots.data(), stride), emit);
        else if (ring_size == 4) dist_scan_column(col, stride, (uint32_t)m, stack.data(), stride, DistRing<4>(slots.data(), stride), emit);
        else if (ring_size == 16) dist_scan_column(col, stride, (uint32_t)m, stack.data(), stride, DistRing<16>(slots.data(), stride), emit);
        else return 2;
        if (!ordered || calls != (uint32_t)m) return 6;
        for (size_t i = 0; i < g.size(); ++i)
            if (i % stride != 0 && (g[i] != -77 || stack[i].value != -77 || stack[i].st != 77u)) return 7;
        for (int32_t u = 0; u < m; ++u) in[(size_t)u] = g[(size_t)u * stride];
        if (fwrite(in.data(), 4, (size_t)m, o) != (size_t)m) return 5;
    }
    fclose(f); fclose(o);
    return 0;
}

static int rows() {
    static char bits[40000];
    uint32_t n, head;
    while (scanf("%" SCNu32 "%" SCNu32 "%39999s", &n, &head, bits) == 3) {
        if (strlen(bits) != n) return 4;
        const uint32_t wpr = (n + head + 31u) / 32u;
        std::vector<uint32_t> words(wpr, 0u);
        for (uint32_t r = 0; r < n; ++r)
            if (bits[r] == '1') words[(r + head) >> 5] |= 1u << ((r + head) & 31u);
        for (uint32_t r = 0; r < n; ++r) printf("%d ", (int)dist_row_nearest(words.data(), wpr, r + head));
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "scan")) return scan(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "rows")) return rows();
    printf("%d %u %" PRIu64 " %zu\n", (int)kDistFar, kDistMaxExtent, kDistMaxVoxels, sizeof(DistEntry));
    for (;;) {
        int64_t n[3]; uint32_t head;
        if (scanf("%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNu32, &n[0], &n[1], &n[2], &head) != 4) return 0;
        DistPlan p; int refused = 0;
        if (!dist_plan(n, head, p, &refused)) { printf(refused == 1 ? "extent\n" : refused == 2 ? "voxels\n" : "empty\n"); continue; }
        printf("%u %u %u %u %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.voxels, p.head, p.wpr, p.upr, p.units, p.columns[0], p.columns[1],
               p.bits_off, p.stack_off, p.bytes);
    }
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("distance_host")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HEADER_DIR,
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def host_scan(exe, tmp_path, columns, stride, ring=16):
    src, out = tmp_path / "columns.bin", tmp_path / "scanned.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(columns)).tobytes())
        for g in columns:
            f.write(np.int32(len(g)).tobytes())
            f.write(np.ascontiguousarray(g, "<i4").tobytes())
    subprocess.run([exe, "scan", str(src), str(out), str(stride), str(ring)], check=True, timeout=120)
    got = np.fromfile(out, "<i4")
    res, at = [], 0
    for g in columns:
        res.append(got[at:at + len(g)])
        at += len(g)
    assert at == len(got)
    return res


def brute(g):
    """min over the i with g[i] != FAR of g[i] + (u - i)^2, in int64; FAR where there is none."""
    g = np.asarray(g, np.int64)
    start = np.where(g == FAR, np.int64(1) << 60, g).reshape(1, 1, -1)
    out = axis_minimum(start, 2).reshape(-1)
    return np.where(out >= np.int64(1) << 60, FAR, out).astype(np.int32)


def test_the_scan_is_brute_force(driver, tmp_path):
    rng = np.random.default_rng(17)
    columns = []
    for m in (1, 2, 63, 64, 65, 1000):
        columns.append(rng.integers(0, 50, m))                              # random g
        columns.append(rng.integers(0, 3 * m * m + 2, m))                   # from no parabola hidden to most of them hidden
        sparse = np.where(rng.random(m) < 0.8, FAR, rng.integers(0, 400, m))
        columns.append(sparse)
        columns.append(np.full(m, FAR))                                     # no source at all
        for end in (0, m - 1):                                              # one finite entry at either end
            one = np.full(m, FAR)
            one[end] = 7
            columns.append(one)
        columns.append(np.full(m, 5))                                       # equal neighbours: every separator is a tie
        columns.append(np.repeat(rng.integers(0, 30, (m + 2) // 3), 3)[:m]) # runs of equal values
        columns.append(np.zeros(m, np.int64))
        columns.append((np.arange(m) - m // 2) ** 2)                        # one parabola owns everything: every other is popped or never starts
        columns.append(np.arange(m)[::-1] ** 2 * 2)
    columns = [np.asarray(c, np.int32) for c in columns]
    want = [brute(g) for g in columns]
    for stride, ring in ((1, 16), (3, 4), (3, 1), (1, 4)):              # the ring the kernel uses, and rings most pops miss
        got = host_scan(driver, tmp_path, columns, stride, ring)
        for g, out, ref in zip(columns, got, want):
            assert np.array_equal(out, ref), (len(g), stride, ring, g[:8])


def test_the_scan_holds_at_the_largest_values(driver, tmp_path):
    """One column of the longest extent with entries near 2 * 2^28, the most the z pass meets (dx^2 + dy^2): parabola
    values reach 3 * 2^28 and the separator's numerator 2^29 + 2^28; both fit int32 (csrc/distance_scan.h)."""
    m, G = MAX_EXTENT, 2 * (MAX_EXTENT - 1) ** 2
    assert G + (m - 1) ** 2 < FAR
    ends = np.full(m, FAR, np.int64)
    ends[0] = ends[-1] = G                                                  # the nearer end owns a position
    u = np.arange(m, dtype=np.int64)
    want_ends = G + np.minimum(u, m - 1 - u) ** 2
    rng = np.random.default_rng(3)
    dense = G - rng.integers(0, 2 ** 20, m)                                 # every entry near the top, few hidden
    steep = np.where(u % 4096 == 0, G - (m - 1) ** 2 // 2, G)               # a few deep parabolas that hide thousands
    low_high = np.where(u < m // 2, 0, G)                                   # the largest difference of two values
    got = host_scan(driver, tmp_path, [ends.astype(np.int32), dense.astype(np.int32), steep.astype(np.int32), low_high.astype(np.int32)], 1)
    assert np.array_equal(got[0], want_ends) and int(got[0].max()) == G + (m // 2 - 1) ** 2
    assert np.array_equal(got[1], brute(dense)) and np.array_equal(got[2], brute(steep))
    assert np.array_equal(got[3], np.where(u < m // 2, 0, (u - (m // 2 - 1)) ** 2))         # the last 0 is the nearest source of the upper half


def test_the_x_pass_is_brute_force(driver):
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 29, 31, 32, 33, 64, 65, 200):
        for head in (0, 1, 3):
            for p in (0.0, 0.02, 0.5, 1.0):
                cases.append((n, head, rng.random(n) < p))
            for end in (0, n - 1):
                one = np.zeros(n, bool)
                one[end] = True
                cases.append((n, head, one))
    text = "".join(f"{n} {head} {''.join('1' if b else '0' for b in bits)}\n" for n, head, bits in cases)
    out = subprocess.run([driver, "rows"], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    for (n, head, bits), line in zip(cases, out):
        want = squared_edt(bits.reshape(1, 1, -1)).reshape(-1)
        assert [int(v) for v in line.split()] == want.tolist(), (n, head)


def plans(exe, cases):
    out = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    res = []
    for line in lines[1:]:
        if line in ("empty", "extent", "voxels"):
            res.append(line)
            continue
        w = [int(v) for v in line.split()]
        res.append(dict(voxels=w[0], head=w[1], wpr=w[2], upr=w[3], units=w[4], columns=w[5:7], bits_off=w[7], stack_off=w[8], bytes=w[9]))
    assert len(res) == len(cases)
    return [int(v) for v in lines[0].split()], res


def test_distance_plan(driver):
    (far, max_extent, max_voxels, entry), _ = plans(driver, [])
    assert (far, max_extent, max_voxels, entry) == (FAR, MAX_EXTENT, 1 << 30, 8) == (N.DISTANCE_FAR, N.DISTANCE_MAX_EXTENT, N.DISTANCE_MAX_VOXELS, 8)
    assert 3 * (max_extent - 1) ** 2 < far                       # every distance fits below FAR
    cases = [(nx, 3, 2, h) for nx in (1, 3, 4, 5, 29, 30, 32, 33, 65) for h in (0, 1, 3)]
    cases += [(MAX_EXTENT, MAX_EXTENT, 4, 3), (1, MAX_EXTENT, MAX_EXTENT, 3), (30, 1 << 12, 1 << 13, 3), (1 << 10, 1 << 10, 1 << 10, 0)]
    # the windows and boxes of tests/test_gpu_odd_rings.py: head is the ring slot modulo 4 of the first voxel (box_head)
    odd = [(*n, lo[0] % ring[0] & 3) for ring, off, lo, n in plan_cases()]
    assert {c[3] for c in odd} == {0, 1, 2, 3} and {1, 3, 63} <= {c[0] for c in odd}
    cases += odd
    _, res = plans(driver, cases)
    for c, p in zip(cases, res):
        nx, ny, nz, head = c
        voxels = nx * ny * nz
        assert p["voxels"] == voxels and p["head"] == head and p["wpr"] == -(-(nx + head) // 32) and p["upr"] == 8 * p["wpr"], (c, p)
        assert p["units"] == p["upr"] * ny * nz < 1 << 32 and 4 * p["upr"] >= nx + head
        assert p["columns"] == [nx * nz, nx * ny]
        # the scratch: the bits, then the stacks at a multiple of 16, 8 bytes per voxel
        assert p["bits_off"] == 0 and p["stack_off"] == -(-(4 * p["wpr"] * ny * nz) // 16) * 16 and p["bytes"] == p["stack_off"] + 8 * voxels


def test_distance_plan_refusals(driver):
    _, res = plans(driver, [(0, 4, 4, 0), (4, -1, 4, 0), (MAX_EXTENT + 1, 1, 1, 0), (1, 1, MAX_EXTENT + 1, 0), (1 << 40, 1 << 40, 1 << 40, 0),
                            ((1 << 10) + 1, 1 << 10, 1 << 10, 0), (MAX_EXTENT, MAX_EXTENT, 5, 0), (MAX_EXTENT, MAX_EXTENT, 4, 0)])
    assert res[:7] == ["empty", "empty", "extent", "extent", "extent", "voxels", "voxels"] and res[7]["voxels"] == 1 << 30


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_distance" in N.SIGNATURES
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert re.search(r"#define SVR_DISTANCE_FAR 0x7FFFFFFF\b", header) and re.search(r"#define SVR_DISTANCE_MAX_EXTENT 16384\b", header)
    assert re.search(r"#define SVR_DISTANCE_MAX_VOXELS \(1u << 30\)", header)
    assert "DistanceField" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "distance")
    import __graft_entry__ as g
    import inspect

    assert "distance_kernels.hip" in g.HIP_SOURCES
    assert "distance_plan.h" in inspect.getsource(g.build_hip) and "distance_scan.h" in inspect.getsource(g.build_hip)


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(svr_distance_params), sizeof(svr_distance_outputs), offsetof(svr_distance_params, selected), "
                   "offsetof(svr_distance_params, invert), offsetof(svr_distance_params, border), offsetof(svr_distance_outputs, d2_capacity), "
                   "offsetof(svr_distance_outputs, header)); return 0; }\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.DistanceParams), C.sizeof(N.DistanceOutputs), N.DistanceParams.selected.offset, N.DistanceParams.invert.offset,
                   N.DistanceParams.border.offset, N.DistanceOutputs.d2_capacity.offset, N.DistanceOutputs.header.offset]
    assert got[:2] == [64, 24]


def test_argument_errors_fire_without_a_gpu():
    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    for kw in (dict(level=0.5, labels=[1]), dict(invert=1), dict(border=None), dict(signed="yes"), dict(labels=[]), dict(labels="12"),
               dict(labels=[-1]), dict(labels=[1.5]), dict(level=float("nan")), dict(level="high"), dict(level=True), dict(lod=1), dict(level=1.0, lod=-1),
               dict(level=1.0, box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4)))):
        with pytest.raises(ValueError):
            vol.distance(**kw)
    assert distance_arguments(None, None, False, False, True, False) == (N.COMPONENTS_LABELS, None, 0.0, 1, 0, 1, False)
    mode, ids, level, ignore_zero, invert, border, signed = distance_arguments(None, [3, 1, 3], True, True, False, True)
    assert (mode, ids.tolist(), ignore_zero, invert, border, signed) == (N.COMPONENTS_LABELS, [1, 3], 0, 1, 0, True)
    assert distance_arguments(7, None, False, False, True, False) == (N.COMPONENTS_LEVEL, None, 7.0, 0, 0, 1, False)
    assert distance_arguments(float("inf"), None, False, False, True, False)[2] == float("inf")


def test_distance_field_answers_on_the_cpu():
    """DistanceField's methods are numpy and torch ops: on CPU tensors they answer from the twin's arrays."""
    import torch

    class World:
        matrix = np.diag([2.0, 1.0, 0.5, 1.0])

    class Volume:
        world = World()

    Volume.world.matrix[:3, 3] = (3.0, -2.0, 7.0)
    rng = np.random.default_rng(5)
    density = rng.random((6, 7, 8)).astype(np.float32)
    density[2:5, 2:6, 2:7] = 1.0                                          # something thick
    off, box = (16, 8, 40), ((17, 8, 41), (6, 7, 4))
    twin = distance_twin(off, density, None, box=box, level=0.6, border=True)
    other = distance_twin(off, density, None, box=box, level=0.6, invert=True)
    head = twin["header"]
    at = head[14]
    deepest = (41 + at // 42, 8 + at // 6 % 7, 17 + at % 6)

    def field(d2, **kw):
        return DistanceField(squared=torch.from_numpy(d2.copy()), begin=(41, 8, 17), offset=off[::-1], inside_voxels=head[1], targets=head[0],
                             far_voxels=head[15], max_squared=head[3], deepest=deepest, lod=1, scale_factor=(0.5, 0.5, 0.25), volume=Volume(), **kw)

    f = field(twin["d2"])
    d2 = twin["d2"].astype(np.int64)
    assert head[3] >= 4 and int(d2[at // 42, at // 6 % 7, at % 6]) == head[3] == int(d2.max())
    assert f.radius() == float(np.sqrt(head[3]))
    assert np.array_equal(f.distance().numpy(), np.sqrt(d2).astype(np.float32)) and f.distance().dtype == torch.float32
    for r in (0, 1, 1.0, 1.5, np.sqrt(2.0), 2, 100):
        assert np.array_equal(f.eroded(r).numpy(), d2 > r * r), r
        assert np.array_equal(f.within(r).numpy(), (d2 > 0) & (d2 <= r * r)), r
        assert f.eroded(r).dtype == torch.bool
    assert np.array_equal(f.eroded(0).numpy(), d2 > 0)                     # the targets themselves
    for bad in (-1, float("nan"), "2", True, None):
        with pytest.raises(ValueError):
            f.eroded(bad)
        with pytest.raises(ValueError):
            f.within(bad)
    # dilation by r: the inside set, or within r of it
    g = field(other["d2"])
    inside = twin["d2"] > 0
    for r in (1, 1.5, 2):
        want = ndimage.distance_transform_edt(~inside) <= r
        assert np.array_equal((g.within(r) | torch.from_numpy(inside)).numpy(), want), r
    # signed: positive inside, negative outside, nothing mixed
    s = signed_squared(torch.from_numpy(twin["d2"]), torch.from_numpy(other["d2"]))
    assert s.dtype == torch.int32 and np.array_equal(s.numpy(), np.where(inside, twin["d2"], -other["d2"]))
    sf = field(s.numpy())
    assert np.array_equal(sf.distance().numpy(), np.where(inside, np.sqrt(d2), -np.sqrt(other["d2"].astype(np.int64))).astype(np.float32))
    assert np.array_equal(sf.eroded(1).numpy(), d2 > 1) and np.array_equal(sf.within(1).numpy(), d2 == 1)
    # FAR on either side stays +-FAR and becomes +-inf
    all_in = np.full((2, 2, 2), FAR, np.int32)
    zero = np.zeros((2, 2, 2), np.int32)
    plus, minus = signed_squared(torch.from_numpy(all_in), torch.from_numpy(zero)), signed_squared(torch.from_numpy(zero), torch.from_numpy(all_in))
    assert bool((plus == FAR).all()) and bool((minus == -FAR).all())
    far = field(np.array([[[FAR, 4, 0, -9, -FAR]]], np.int32))
    assert far.distance().numpy().tolist() == [[[float("inf"), 2.0, 0.0, -3.0, float("-inf")]]]
    assert far.eroded(1e9).numpy().tolist() == [[[True, False, False, False, False]]]
    assert far.within(1e9).numpy().tolist() == [[[False, True, False, False, False]]]
    # the deepest voxel as a world position, and the depth under a picked point
    c = np.array(deepest[::-1], np.float64)                               # shader order
    world = ((c + 0.5) / np.array([0.25, 0.5, 0.5]) - 0.5) * np.array([2.0, 1.0, 0.5]) + np.array([3.0, -2.0, 7.0])
    assert np.allclose(f.deepest_position(), world, rtol=0, atol=1e-12) and f.at(f.deepest_position()) == head[3]
    z, y, x = np.meshgrid(*[np.arange(n) for n in twin["d2"].shape], indexing="ij")
    for dz, dy, dx in ((0.0, 0.0, 0.0), (0.4, -0.4, 0.4)):
        for k in rng.integers(0, z.size, 40):
            c = np.array([x.flat[k] + 17 + dx, y.flat[k] + 8 + dy, z.flat[k] + 41 + dz])
            world = ((c + 0.5) / np.array([0.25, 0.5, 0.5]) - 0.5) * np.array([2.0, 1.0, 0.5]) + np.array([3.0, -2.0, 7.0])
            assert f.at(world) == int(twin["d2"].flat[k])
    assert f.at((-1000.0, 0.0, 0.0)) == 0 and f.at((1e6, 1e6, 1e6)) == 0
