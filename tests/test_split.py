"""No GPU: the contract of svr_split (include/svr.h) as tests/split_twin.py restates it, held to a brute force in pure
Python, to known answers on balls and plateaus and to scipy; the link predicate, the plan and the union-find over summits
of the kernels' own headers (split_link.h, split_plan.h, components_uf.h), compiled into a host program under ASan and
UBSan; the structs; the Python surface."""
import ctypes as C
import os
import re
import shutil
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest
from scipy import ndimage

from distance_twin import FAR, squared_edt
from split_twin import MAX_MERGE, RECORD, count_only, links, split_brute, split_twin, summits_of
from parent_plans import held_to_parent
from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial, _native as N
from sub_volume_renderer_amd.split import SplitLabels, split_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
MERGES = (0, 1, 4, 1 << 29)


def balls(shape, centres, r):
    """bool [z][y][x]: the voxels within r of one of the centres (z, y, x)."""
    z, y, x = np.indices(shape)
    m = np.zeros(shape, bool)
    for c in centres:
        m |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return m


def depth(inside):
    return squared_edt(~inside, border=True)


def same_partition(a, b):
    """Do two volumes of numbers (0 outside) cut the voxels into the same sets?"""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    if not np.array_equal(a == 0, b == 0):
        return False
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- the twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_twin_is_brute_force(connectivity):
    rng = np.random.default_rng(31)
    shapes = [(1, 1, 1), (1, 1, 5), (7, 1, 1), (2, 3, 4), (6, 7, 8), (5, 7, 8), (6, 6, 7), (3, 7, 8)]     # (z, y, x): up to 8 x 7 x 6
    several = 0
    for shape in shapes:
        for trial in range(3):
            height = (rng.integers(0, 4, shape) * (rng.random(shape) < 0.7)).astype(np.int32)           # about half zeros, many ties
            if trial == 2:
                height = np.where(height == 3, FAR, height).astype(np.int32)
            for H in MERGES:
                twin = split_twin(height, connectivity, H)
                ids, records, basins = split_brute(height.tolist(), connectivity, H)
                what = (shape, trial, H)
                assert np.array_equal(twin["ids"], np.array(ids, np.uint32).reshape(shape)), what
                assert twin["header"] == [len(records), int((height > 0).sum()), height.size, len(records), basins, 0, 0, 0, 0, 0,
                                          shape[2], shape[1], shape[0], 0, 0, 0], what
                assert len(twin["records"]) == len(records)
                for want, got in zip(records, twin["records"]):
                    for name in RECORD.names:
                        assert np.array_equal(np.array(want[name]), got[name]), (what, name)
                several += len(records) > 2
    assert several > 20
    assert count_only([5, 9, 60, 5, 7] + [0] * 5 + [5, 4, 3, 0, 0, 0]) == [5, 9, 0, 0, 7] + [0] * 5 + [5, 4, 3, 0, 0, 0]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_two_balls_of_radius_6(connectivity):
    centres = [(8, 8, 8), (8, 8, 17)]
    inside = balls((16, 16, 26), centres, 6)
    d2 = depth(inside)
    assert int(inside.sum()) == 1774
    for H, regions in ((0, 2), (1, 2), (4, 1), (1 << 29, 1)):
        twin = split_twin(d2, connectivity, H)
        assert twin["header"][:2] == [regions, 1774], H
        if regions == 2:
            # every voxel that is not equidistant from the two centres' x belongs to the nearer centre's region
            x = np.indices(d2.shape)[2]
            left, right = inside & (2 * x < 8 + 17), inside & (2 * x > 8 + 17)
            assert left.sum() + right.sum() == 1774                      # 8 + 17 is odd: no voxel is equidistant
            a, b = int(twin["ids"][8, 8, 8]), int(twin["ids"][8, 8, 17])
            assert {a, b} == {1, 2}
            assert int((twin["ids"][left] != a).sum()) + int((twin["ids"][right] != b).sum()) == 0
            # 37 = 6^2 + 1^2: the nearest lattice point beyond a ball of radius 6
            assert twin["records"]["top"].tolist() == [[8, 8, 8], [17, 8, 8]] and twin["records"]["peak"].tolist() == [37, 37]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_two_balls_of_radius_8_and_one_ball(connectivity):
    d2 = depth(balls((20, 20, 32), [(10, 10, 10), (10, 10, 22)], 8))
    assert [split_twin(d2, connectivity, H)["header"][0] for H in MERGES] == [2, 2, 2, 1]
    d2 = depth(balls((15, 15, 15), [(7, 7, 7)], 6))
    for H in MERGES:
        twin = split_twin(d2, connectivity, H)
        # four equal summits around the centre under 6-connectivity: the plateau rule, not luck, gives one region
        assert twin["header"][0] == 1 and twin["header"][4] == (4 if connectivity == 6 else 1), H
        assert twin["records"]["basins"].tolist() == [twin["header"][4]] and twin["records"]["voxels"].tolist() == [925]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_plateaus_are_one_region(connectivity):
    solid = np.full((5, 6, 7), FAR, np.int32)
    twin = split_twin(solid, connectivity, 0)
    assert twin["header"][:2] == [1, 210] and twin["records"]["peak"].tolist() == [FAR] and twin["records"]["top"].tolist() == [[0, 0, 0]]
    u = np.zeros((3, 7, 9), np.int32)
    u[1, 1:6, 1] = u[1, 1:6, 7] = u[1, 5, 1:8] = 5                          # a U in one plane: its two arms meet far from their tips
    twin = split_twin(u, connectivity, 0)
    assert twin["header"][0] == 1 and twin["header"][1] == int((u > 0).sum()) and twin["header"][4] >= 2
    assert twin["records"]["top"].tolist() == [[1, 1, 1]] and twin["records"]["lo"].tolist() == [[1, 1, 1]] and twin["records"]["hi"].tolist() == [[7, 5, 1]]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_largest_merge_gives_the_components_of_scipy(connectivity):
    rng = np.random.default_rng(8)
    structure = None if connectivity == 6 else np.ones((3, 3, 3))
    for shape in ((6, 7, 8), (9, 10, 11), (1, 12, 12)):
        for fill in (0.3, 0.5, 0.8):
            height = (rng.integers(1, 40, shape) * (rng.random(shape) < fill)).astype(np.int32)
            twin = split_twin(height, connectivity, MAX_MERGE)
            want, count = ndimage.label(height > 0, structure=structure)
            assert twin["header"][0] == count and same_partition(twin["ids"], want), (shape, fill)
            assert split_twin(height, connectivity, 0)["header"][0] >= count
    assert not same_partition([1, 1, 2], [1, 2, 2]) and same_partition([0, 2, 1, 1], [0, 1, 3, 3]) and not same_partition([0, 1], [1, 1])


# ---- the kernels' own headers on the host ----------------------------------------------------------------------------------
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "split_link.h"
#include "split_plan.h"
#include "components_uf.h"

// links: lines of "a s H" -> a line of 0 / 1 each
static int do_links() {
    long long a, s, H;
    while (scanf("%lld %lld %lld", &a, &s, &H) == 3) printf("%d\n", split_links((int32_t)a, (int32_t)s, (uint32_t)H) ? 1 : 0);
    return 0;
}

// plans: lines of "nx ny nz" -> the plan, or "refused"
static int do_plans() {
    printf("%u %u %d %" PRIu64 " %u\n", kSplitOutside, kBoxScanBlock, kBoxScanMaxLevels, kSplitMaxVoxels, kSplitMaxMerge);
    long long n[3];
    while (scanf("%lld %lld %lld", &n[0], &n[1], &n[2]) == 3) {
        const int32_t m[3] = {(int32_t)n[0], (int32_t)n[1], (int32_t)n[2]};
        SplitPlan p;
        if (!split_plan(m, p)) { printf("refused\n"); continue; }
        printf("%u %d %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64, p.voxels, (int)p.scan.levels, p.scan.count[0], p.scan.count[1], p.scan.count[2],
               p.up_off, p.uf_off, p.aux_off);
        for (int k = 0; k < 3; ++k) printf(" %" PRIu64, p.scan.off[k]);
        printf(" %" PRIu64 " %u %" PRIu64 "\n", p.bytes, p.scan.count[3], p.scan.off[3]);
    }
    return 0;
}

// regions in nx ny nz conn H threads out: the file holds height (int32) then summit (uint32) per voxel, kSplitOutside
// where the voxel is outside.  What split_link_kernel does, with `threads` threads over interleaved voxels: the
// neighbours before a voxel, split_links, uf_union over an array in which only summits are entries.  Then the flatten.
static int do_regions(char** argv) {
    const uint32_t nx = (uint32_t)atoi(argv[3]), ny = (uint32_t)atoi(argv[4]), nz = (uint32_t)atoi(argv[5]);
    const int conn = atoi(argv[6]);
    const uint32_t H = (uint32_t)strtoul(argv[7], nullptr, 10);
    const unsigned threads = (unsigned)atoi(argv[8]);
    const uint32_t voxels = nx * ny * nz;
    std::vector<int32_t> height(voxels);
    std::vector<uint32_t> summit(voxels), uf(voxels);
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(height.data(), 4, voxels, f) != voxels || fread(summit.data(), 4, voxels, f) != voxels) return 4;
    fclose(f);
    for (uint32_t i = 0; i < voxels; ++i) uf[i] = summit[i] == i ? i : kUfOutside;
    auto work = [&](unsigned t) {
        for (uint32_t i = t; i < voxels; i += threads) {
            const uint32_t si = summit[i];
            if (si == kSplitOutside) continue;
            const uint32_t x = i % nx, y = i / nx % ny, z = i / nx / ny;
            for (int dz = -1; dz <= 0; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
                if (!(dz < 0 || dy < 0 || (dy == 0 && dx < 0))) continue;
                if (conn == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy, qz = z + (uint32_t)dz;
                if (qx >= nx || qy >= ny || qz >= nz) continue;
                const uint32_t j = (qz * ny + qy) * nx + qx, sj = summit[j];
                if (sj == kSplitOutside || sj == si) continue;
                const int32_t a = height[si] < height[sj] ? height[si] : height[sj], s = height[i] < height[j] ? height[i] : height[j];
                if (split_links(a, s, H)) uf_union(uf.data(), si, sj);
            }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
    for (uint32_t i = 0; i < voxels; ++i) {
        if (uf[i] == kUfOutside) continue;
        (void)uf_min(uf.data() + i, uf_find(uf.data(), i));
    }
    FILE* o = fopen(argv[9], "wb");
    if (!o || fwrite(uf.data(), 4, voxels, o) != voxels) return 5;
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "links")) return do_links();
    if (argc > 1 && !strcmp(argv[1], "plans")) return do_plans();
    if (argc > 9 && !strcmp(argv[1], "regions")) return do_regions(argv);
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("split_host")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def exact_links(a, s, H):
    """sqrt(a) - sqrt(s) <= sqrt(H) for integers a >= s >= 1, H >= 0, in Python's unbounded integers: moving sqrt(s)
    over and squaring twice, each time between sides that are not negative."""
    t = a - s - H                      # sqrt(a) <= sqrt(s) + sqrt(H)  <=>  a <= s + H + 2 sqrt(H s)  <=>  t <= 2 sqrt(H s)
    return t <= 0 or t * t <= 4 * H * s


def test_the_link_predicate_is_the_exact_test(driver):
    cases = []
    for H in (0, 1, 4, 9, 1000, 1 << 29):
        # the equality boundary t^2 = 4 H s: s = H k^2, a = H (k + 1)^2, where sqrt(a) - sqrt(s) = sqrt(H); and one either side
        for k in (1, 2, 3, 7, 100, 1000, 46339):
            s, a = H * k * k, H * (k + 1) * (k + 1)
            for da in (-1, 0, 1):
                if 1 <= s <= a + da <= FAR:
                    cases.append((a + da, s, H))
        for s in (1, 2, 3, 50, 3 << 28, FAR):
            for a in (s, s + 1, s + H, 3 << 28, FAR, FAR - 1):
                if s <= a <= FAR:
                    cases.append((a, s, H))
        cases += [(FAR, 1, H), (3 << 28, 1, H), (FAR, 3 << 28, H), (FAR, FAR, H)]
    rng = np.random.default_rng(3)
    for _ in range(3000):
        s = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        a = min(FAR, s + int(rng.integers(0, 1 << int(rng.integers(1, 32)))))
        cases.append((a, min(s, a), int(rng.integers(0, (1 << 29) + 1))))
    out = subprocess.run([driver, "links"], input="".join(f"{a} {s} {H}\n" for a, s, H in cases), capture_output=True, text=True, check=True)
    got = [int(v) for v in out.stdout.split()]
    assert len(got) == len(cases)
    getcontext().prec = 80
    boundary = 0
    for (a, s, H), g in zip(cases, got):
        want = exact_links(a, s, H)
        assert bool(g) == want, (a, s, H)
        assert bool(links(np.int64(a), np.int64(s), np.int64(H))) == want, (a, s, H)       # the twin's, in int64
        t = a - s - H
        if t > 0 and t * t == 4 * H * s:
            boundary += 1
            assert want                                                  # equality links
        else:                                                            # away from equality the roots themselves decide, to 80 digits
            assert (Decimal(a).sqrt() - Decimal(s).sqrt() <= Decimal(H).sqrt()) == want, (a, s, H)
    assert boundary >= 20 and 0 < sum(got) < len(got)
    assert exact_links(5, 5, 0) and not exact_links(6, 5, 0) and exact_links(4, 1, 1) and not exact_links(5, 1, 1)


def test_split_plan(driver):
    cases = [(1, 1, 1), (5, 1, 1), (256, 1, 1), (257, 1, 1), (67, 33, 31), (256, 256, 1), (257, 255, 1), (1024, 1024, 1024), (512, 512, 512),
             (0, 4, 4), (4, -1, 4), (1024, 1024, 1025), (2147483647, 2147483647, 2147483647), (1 << 30, 1, 1), ((1 << 30) + 1, 1, 1)]
    out = subprocess.run([driver, "plans"], input="".join(f"{a} {b} {c}\n" for a, b, c in cases), capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    assert lines[0].split() == [str(0xFFFFFFFF), "256", "4", str(1 << 30), str(1 << 29)]
    for n, line in zip(cases, lines[1:]):
        voxels = n[0] * n[1] * n[2]
        if min(n) <= 0 or voxels > 1 << 30:
            assert line == "refused", n
            continue
        v = [int(t) for t in line.split()]
        count = [-(-voxels // 256)]
        while count[-1] > 256:
            count.append(-(-count[-1] // 256))
        levels = len(count)
        count += [0] * (3 - levels)
        offs, at = [], 12 * voxels
        for k in range(3):
            offs.append(at)
            at += 4 * count[k]
        # the fourth level, which 2^30 voxels never need, takes no bytes; and nothing moved
        assert v == [voxels, levels, *count, 0, 4 * voxels, 8 * voxels, *offs, at, 0, at], n
        held_to_parent("split", n, v[5:12])
        # 12 bytes per voxel plus the scan levels, each a 256th of the one below, rounded up
        assert at <= 12 * voxels + 4 * (voxels // 256 + voxels // 65536 + voxels // (1 << 24) + 3)
    assert len(lines) == 1 + len(cases)
    # 68,541 voxels: the smallest box of the GPU tests whose scan has a second level (268 counts > 256)
    assert 67 * 33 * 31 == 68541 and -(-68541 // 256) == 268


@pytest.mark.parametrize("connectivity", [6, 26])
def test_union_find_over_summits_with_8_threads(driver, tmp_path, connectivity):
    rng = np.random.default_rng(44)
    fields = [("random", (rng.integers(0, 4, (24, 20, 35)) * (rng.random((24, 20, 35)) < 0.7)).astype(np.int32)),
              ("balls", depth(balls((20, 20, 32), [(10, 10, 10), (10, 10, 22), (4, 4, 16)], 8))),
              ("plateau", np.full((5, 6, 7), FAR, np.int32)),
              ("ridges", (rng.integers(1, 3, (9, 30, 30)) * (np.indices((9, 30, 30)).sum(axis=0) % 3 > 0)).astype(np.int32))]
    joined = 0
    for name, height in fields:
        nz, ny, nx = height.shape
        for H in (0, 1, 9, 1 << 29):
            twin = split_twin(height, connectivity, H)
            inside, summit = summits_of(height, connectivity)
            flat = np.where(inside, summit, 0xFFFFFFFF).astype("<u4").reshape(-1)
            is_summit = flat == np.arange(height.size)
            want = np.full(height.size, 0xFFFFFFFF, np.uint32)
            want[is_summit] = twin["seeds"][twin["ids"].reshape(-1)[is_summit].astype(np.int64) - 1]
            joined += int(is_summit.sum()) - twin["header"][0]
            src = tmp_path / "field.bin"
            with open(src, "wb") as f:
                f.write(np.ascontiguousarray(height, "<i4").tobytes())
                f.write(flat.tobytes())
            for threads in (1, 8):
                out = tmp_path / "uf.bin"
                subprocess.run([driver, "regions", str(src), str(nx), str(ny), str(nz), str(connectivity), str(H), str(threads), str(out)],
                               check=True, timeout=120)
                assert np.array_equal(np.fromfile(out, "<u4"), want), (name, H, threads)
    assert joined > 1000                                                 # unions were made, many of them


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_split" in N.SIGNATURES
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert re.search(r"#define SVR_SPLIT_MAX_VOXELS \(1u << 30\)", header) and re.search(r"#define SVR_SPLIT_MAX_MERGE  \(1u << 29\)", header)
    assert (N.SPLIT_MAX_VOXELS, N.SPLIT_MAX_MERGE, N.SPLIT_RECORD_BYTES) == (1 << 30, 1 << 29, 80) == (1 << 30, MAX_MERGE, RECORD.itemsize)
    assert "SplitLabels" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "split")
    import __graft_entry__ as g
    import inspect

    assert "split_kernels.hip" in g.HIP_SOURCES
    assert "split_plan.h" in inspect.getsource(g.build_hip) and "split_link.h" in inspect.getsource(g.build_hip)
    params = inspect.signature(SubVolume.split).parameters
    assert list(params)[1:] == ["level", "labels", "background", "merge", "connectivity", "border", "lod", "box", "distance", "stream"]
    assert (params["merge"].default, params["connectivity"].default, params["border"].default) == (1.0, 26, True)


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    fields = [("svr_split_params", N.SplitParams), ("svr_split_record", N.SplitRecord), ("svr_split_outputs", N.SplitOutputs)]
    prints, want = [], []
    for name, struct in fields:
        prints.append(f"sizeof({name})")
        want.append(C.sizeof(struct))
        for field, _ in struct._fields_:
            prints.append(f"offsetof({name}, {field})")
            want.append(getattr(struct, field).offset)
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu\\n", {p});\n' for p in prints) + "    return 0;\n}\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(N.SplitRecord) == 80 == RECORD.itemsize and C.sizeof(N.SplitParams) == 32 and C.sizeof(N.SplitOutputs) == 40
    assert [RECORD.fields[name][1] for name in RECORD.names] == [getattr(N.SplitRecord, name).offset for name, _ in N.SplitRecord._fields_]
    assert N.SplitRecord.top.offset % 8 == 0                            # the emit pass keeps a 64-bit maximum there


def test_argument_errors_fire_without_a_gpu():
    import torch

    from sub_volume_renderer_amd.distance import DistanceField

    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    field = DistanceField(squared=torch.zeros((2, 2, 2), dtype=torch.int32), begin=(0, 0, 0), offset=(0, 0, 0), inside_voxels=0, targets=0,
                          far_voxels=0, max_squared=0, deepest=(0, 0, 0), lod=0)
    for kw in (dict(level=1.0, connectivity=18), dict(level=1.0, connectivity=True), dict(level=1.0, merge=-1), dict(level=1.0, merge="2"),
               dict(level=1.0, merge=float("nan")), dict(level=1.0, merge=23171), dict(level=1.0, merge=True), dict(distance=field, level=1.0),
               dict(distance=field, labels=[1]), dict(distance=np.zeros((2, 2, 2), np.int32)), dict(distance=field),       # a CPU tensor
               dict(level=0.5, labels=[1]), dict(level=float("nan")), dict(level=1.0, lod=4), dict(level=1.0, border=1)):
        with pytest.raises(ValueError):
            vol.split(**kw)
    assert split_arguments(None, None, 1.0, 26, None) == (1, 26)
    assert split_arguments(3.0, None, 2.5, 6, None) == (6, 6) and split_arguments(None, [1], 0, 6, None) == (0, 6)
    assert split_arguments(None, None, 23170, 26, field) == (23170 * 23170, 26) and 23170 * 23170 <= MAX_MERGE < 23171 * 23171


def test_split_labels_answer_on_the_cpu():
    """SplitLabels' methods are numpy and torch ops: on CPU tensors they answer from the twin's arrays."""
    import torch

    class World:
        matrix = np.diag([2.0, 1.0, 0.5, 1.0])

    class Volume:
        world = World()

    Volume.world.matrix[:3, 3] = (3.0, -2.0, 7.0)
    d2 = depth(balls((16, 16, 26), [(8, 8, 8), (8, 8, 17)], 6))
    twin = split_twin(d2, 26, 1)
    rec, begin, scale = twin["records"], np.array((41, 8, 17)), (0.5, 0.5, 0.25)
    t = lambda a, dtype=torch.int64: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    labels = SplitLabels(ids=t(twin["ids"].astype(np.int32), torch.int32), count=2, basins=twin["header"][4], begin=tuple(begin), offset=(40, 8, 16),
                         inside_voxels=1774, voxels=t(rec["voxels"].astype(np.int64)), region_basins=t(rec["basins"].astype(np.int64)),
                         peak_squared=t(rec["peak"].astype(np.int64)), top=t(begin + rec["top"][:, ::-1]), lo=t(begin + rec["lo"][:, ::-1]),
                         end=t(begin + rec["hi"][:, ::-1] + 1), centroid=t(begin + (rec["sum"] / rec["voxels"][:, None])[:, ::-1], torch.float64), lod=2,
                         scale_factor=scale, volume=Volume())
    assert len(labels) == 2 and labels.radius(1) == float(np.sqrt(37.0)) == labels.radius(2)
    for k in (1, 2):
        lo, end = begin + rec["lo"][k - 1][::-1], begin + rec["hi"][k - 1][::-1] + 1
        assert labels.box(k) == (tuple(int(v) for v in np.floor(lo / scale)), tuple(int(v) for v in np.ceil(end / scale)))
        top = begin + rec["top"][k - 1][::-1]                           # (z, y, x)
        data = (top + 0.5) / np.array(scale) - 0.5
        want = (2.0 * data[2] + 3.0, 1.0 * data[1] - 2.0, 0.5 * data[0] + 7.0)
        assert labels.position(k) == pytest.approx(want, abs=1e-12)
        assert labels.id_at(labels.position(k)) == k
        assert np.array_equal(labels.mask(k).numpy(), twin["ids"] == k)
    assert np.array_equal(labels.mask([1, 2]).numpy(), twin["ids"] != 0)
    order = sorted((1, 2), key=lambda k: (-int(rec["voxels"][k - 1]), k))
    assert labels.largest(1) == order[:1] and labels.largest(5) == order and labels.largest(0) == []
    assert labels.id_at((1e6, 0.0, 0.0)) == 0
    for bad in (0, 3, 1.0, True):
        with pytest.raises(KeyError):
            labels.box(bad)
    far = SplitLabels(ids=t(np.ones((1, 1, 1), np.int32), torch.int32), count=1, basins=1, begin=(0, 0, 0), offset=(0, 0, 0), inside_voxels=1,
                      voxels=t(np.array([1])), region_basins=t(np.array([1])), peak_squared=t(np.array([FAR])), top=t(np.zeros((1, 3), np.int64)),
                      lo=t(np.zeros((1, 3), np.int64)), end=t(np.ones((1, 3), np.int64)), centroid=t(np.zeros((1, 3)), torch.float64), lod=0)
    assert far.radius(1) == float("inf")
