"""svr_nearest without a GPU: the numpy restatement (tests/nearest_twin.py) held to an all-pairs brute force with the tie
rule (the minimum distance, then the smallest dense index), to tests/distance_twin.py and to
scipy.ndimage.distance_transform_edt; the owner-reporting scan, the row function with position and the plan
(csrc/distance_scan.h, csrc/distance_plan.h) compiled with the host compiler, address and undefined-behaviour sanitizers
on, into a program of its own that is run directly, and compared with brute force; and the pins of the new surface (the
symbol, the struct sizes, the argument errors of ``SubVolume.nearest``, the arithmetic of ``NearestField``)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from distance_twin import FAR, count_only, distance_twin
from nearest_twin import brute_force, expanded, feature_transform, nearest_twin, tied
from sub_volume_renderer_amd import NearestField, SubVolume, SubVolumeMaterial, _native as N
from sub_volume_renderer_amd.nearest import nearest_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
MAX_EXTENT = 16384
NO_OWNER = 0xFFFF


def boxes():
    """(name, source bool [z][y][x])"""
    rng = np.random.default_rng(41)
    out = []
    for k in range(60):
        shape = tuple(int(v) for v in rng.integers(1, 9, 3))
        if k < 7:                                                       # extents of 1 on every axis, pair of axes and all three
            shape = tuple(1 if (k + 1) >> a & 1 else shape[a] for a in range(3))
        out.append((f"random {k} {shape}", rng.random(shape) < (0.05, 0.2, 0.5)[k % 3]))
    z, y, x = np.meshgrid(np.arange(6), np.arange(7), np.arange(8), indexing="ij")
    out.append(("checkerboard", (x + y + z) % 2 == 0))
    mirrored = np.zeros((5, 5, 7), bool)
    mirrored[2, 2, 1] = mirrored[2, 2, 5] = mirrored[0, 2, 3] = mirrored[4, 2, 3] = mirrored[2, 0, 3] = mirrored[2, 4, 3] = True
    out.append(("mirrored about (2, 2, 3)", mirrored))
    plane = np.zeros((6, 7, 8), bool)
    plane[:, 3, :] = True
    out.append(("one plane", plane))
    out.append(("no source", np.zeros((3, 4, 5), bool)))
    out.append(("all sources", np.ones((3, 4, 5), bool)))
    return out


# ---- the twin ------------------------------------------------------------------------------------------------------------
def test_twin_is_the_brute_force_with_the_tie_rule():
    ties = 0
    for name, source in boxes():
        d2, index = feature_transform(source)
        want_d2, want_index = brute_force(source)
        assert d2.dtype == index.dtype == np.int32
        assert np.array_equal(d2, want_d2) and np.array_equal(index, want_index), name
        ties += int(tied(source).sum())
        if not source.any():
            assert (index == -1).all() and (d2 == FAR).all()
        else:
            own = np.arange(source.size).reshape(source.shape)
            assert np.array_equal(index[source], own[source]) and (index >= 0).all()
    assert ties > 500                                                   # the rule was needed
    source = dict(boxes())["mirrored about (2, 2, 3)"]
    assert tied(source)[2, 2, 3] and feature_transform(source)[1][2, 2, 3] == (0 * 5 + 2) * 7 + 3       # six at distance 2: the smallest z
    source = dict(boxes())["checkerboard"]
    assert tied(source)[1:-1, 1:-1, 1:-1][~source[1:-1, 1:-1, 1:-1]].all()                              # six neighbours each


def test_twin_agrees_with_the_distance_twin_and_scipy():
    rng = np.random.default_rng(12)
    labels = rng.integers(0, 4, (6, 7, 8)).astype(np.uint32)
    labels[labels == 3] = 0xFFFFFFF0
    density = rng.random((6, 7, 8)).astype(np.float32)
    density[1, 2, 3] = np.nan
    off = (16, 8, 40)
    modes = [dict(level=0.6), dict(level=0.9, invert=True), dict(), dict(ignore_zero=True), dict(ignore_zero=True, invert=True),
             dict(selected=[2, 9], ignore_zero=True, invert=True), dict(level=0.5, box=((10, 10, 42), (9, 3, 100))), dict(box=((0, 0, 0), (5, 5, 5))),
             dict(selected=[77], invert=True), dict(level=2.0)]
    for mode in modes:
        for lab in (labels, None):
            twin = nearest_twin(off, density, lab, **mode)
            dist = distance_twin(off, density, lab, border=False, **mode)
            assert twin["header"] == dist["header"] and np.array_equal(twin["d2"], dist["d2"]) and twin["d2"].dtype == np.int32, mode
            assert twin["index"].shape == twin["label"].shape == twin["d2"].shape and twin["label"].dtype == np.uint32
            if not twin["d2"].size:
                continue
            nz, ny, nx = twin["d2"].shape
            far = twin["d2"] == FAR
            assert np.array_equal(twin["index"] == -1, far) and not twin["label"][far].any()
            target = twin["d2"] > 0
            z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
            i = np.maximum(twin["index"], 0).astype(np.int64)
            to_index = (z - i // (ny * nx)) ** 2 + (y - i // nx % ny) ** 2 + (x - i % nx) ** 2
            assert np.array_equal(to_index[~far], twin["d2"][~far])
            if (~target).any() and not far.any():
                edt, (sz, sy, sx) = ndimage.distance_transform_edt(target, return_indices=True)
                assert np.array_equal(np.rint(ndimage.distance_transform_edt(target, return_indices=False) ** 2).astype(np.int64), to_index)
                assert np.array_equal((z - sz) ** 2 + (y - sy) ** 2 + (x - sx) ** 2, to_index)      # scipy's tie choice is its own
            if lab is None:
                assert not twin["label"].any()
            else:
                cut = lab[twin["header"][9] - off[2]:, twin["header"][8] - off[1]:, twin["header"][7] - off[0]:][:nz, :ny, :nx]
                assert np.array_equal(twin["label"][~far], cut.reshape(-1)[i[~far]])
    grown = nearest_twin(off, density, labels, ignore_zero=True, invert=True)
    assert np.array_equal(grown["label"][labels != 0], labels[labels != 0]) and (grown["label"] != 0).all() and (grown["label"] == 0xFFFFFFF0).any()
    assert nearest_twin((3, 4, 5), None, None, level=1.0)["header"] == [0, 0, 0, 0, 3, 4, 5] + [0] * 9


# ---- the scan with owners, the row function with position and the plan on the host ----------------------------------------------
# "scan IN OUT stride ring": as the driver of tests/test_distance.py; OUT receives per column its m values, then its m owners.
# "rows": reads "n head bits" lines -> a line of n "d2:voxel" pairs each (voxel -1 with FAR).
# "plan": reads "nx ny nz head" lines -> "voxels dist_bytes own_off[3] bytes", "empty", "extent" or "voxels".
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
        std::vector<int32_t> in((size_t)m), who((size_t)m, -5);
        if (fread(in.data(), 4, (size_t)m, f) != (size_t)m) return 4;
        std::vector<int32_t> g(((size_t)m - 1) * stride + 1, -77);
        std::vector<DistEntry> stack(((size_t)m - 1) * stride + 1, DistEntry{-77, 77u});
        for (int32_t u = 0; u < m; ++u) g[(size_t)u * stride] = in[(size_t)u];
        int32_t* col = g.data();
        uint32_t calls = 0, last = (uint32_t)m;
        bool ordered = true;
        auto emit = [&](uint32_t u, int32_t v, uint32_t s) {
            ordered = ordered && u + 1u == last; last = u; ++calls;
            col[(size_t)u * stride] = v;
            who[u] = (int32_t)s;
        };
        std::vector<DistEntry> slots(((size_t)ring_size - 1) * stride + 1, DistEntry{-77, 77u});
        if (ring_size == 1) dist_scan_column_owner(col, stride, (uint32_t)m, stack.data(), stride, DistRing<1>(slots.data(), stride), emit);
        else if (ring_size == 16) dist_scan_column_owner(col, stride, (uint32_t)m, stack.data(), stride, DistRing<16>(slots.data(), stride), emit);
        else return 2;
        if (!ordered || calls != (uint32_t)m) return 6;
        for (size_t i = 0; i < g.size(); ++i)
            if (i % stride != 0 && (g[i] != -77 || stack[i].value != -77 || stack[i].st != 77u)) return 7;
        for (int32_t u = 0; u < m; ++u) in[(size_t)u] = g[(size_t)u * stride];
        if (fwrite(in.data(), 4, (size_t)m, o) != (size_t)m || fwrite(who.data(), 4, (size_t)m, o) != (size_t)m) return 5;
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
        for (uint32_t r = 0; r < n; ++r) {
            uint32_t at = 0xDEADu;
            const int32_t d = dist_row_nearest_at(words.data(), wpr, r + head, &at);
            if (d != dist_row_nearest(words.data(), wpr, r + head)) return 8;
            if (d == kDistFar && at != 0xDEADu) return 9;
            printf("%d:%d ", (int)d, d == kDistFar ? -1 : (int)at - (int)head);
        }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "scan")) return scan(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "rows")) return rows();
    printf("%u %u\n", kDistNoOwner, kDistMaxExtent);
    for (;;) {
        int64_t n[3]; uint32_t head;
        if (scanf("%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNu32, &n[0], &n[1], &n[2], &head) != 4) return 0;
        NearPlan p; DistPlan d; int refused = 0, refused_d = 0;
        const bool any = near_plan(n, head, p, &refused);
        if (any != dist_plan(n, head, d, &refused_d) || refused != refused_d) return 3;
        if (!any) { printf(refused == 1 ? "extent\n" : refused == 2 ? "voxels\n" : "empty\n"); continue; }
        if (memcmp(&p.d, &d, sizeof d) != 0) return 3;
        printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.d.voxels, p.d.bytes, p.own_off[0], p.own_off[1], p.own_off[2], p.bytes);
    }
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("nearest_host")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HEADER_DIR,
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def host_scan(exe, tmp_path, columns, stride, ring):
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
        res.append((got[at:at + len(g)], got[at + len(g):at + 2 * len(g)]))
        at += 2 * len(g)
    assert at == len(got)
    return res


def brute_column(g):
    """(min over the i with g[i] != FAR of g[i] + (u - i)^2, the smallest such i) in int64; (FAR, NO_OWNER) where there is none."""
    g = np.asarray(g, np.int64)
    m = len(g)
    u = np.arange(m, dtype=np.int64)
    f = np.where(g[None, :] == FAR, np.int64(1) << 60, g[None, :] + (u[:, None] - u[None, :]) ** 2)       # [u][i]
    value, who = f.min(axis=1), f.argmin(axis=1)                        # argmin keeps the first of equals
    none = value >= np.int64(1) << 60
    return np.where(none, FAR, value).astype(np.int32), np.where(none, NO_OWNER, who).astype(np.int32)


def test_the_scan_names_the_first_owner(driver, tmp_path):
    rng = np.random.default_rng(23)
    G = 2 * (MAX_EXTENT - 1) ** 2                                       # 2 * 2^28, about: the most the z pass meets
    columns = []
    for m in (1, 2, 3, 17, 64, 300):
        i = np.arange(m, dtype=np.int64)
        columns.append(np.zeros(m, np.int64))                           # every position its own
        columns.append(np.full(m, 9))                                   # all equal
        columns.append(i ** 2)                                          # g[i] = i^2: i and 0 tie at every position u = i... and more
        columns.append(np.where(i % 2 == 0, i % 7, FAR))                # every second entry FAR
        columns.append(np.where(i % 2 == 1, 3, FAR))
        columns.append(np.full(m, FAR))                                 # all FAR
        columns.append(np.full(m, G))                                   # the largest values
        columns.append(G - (i % 5) * 1000)
        columns.append(np.where(i < m // 2, 0, G))
        columns.append(rng.integers(0, 40, m))
        columns.append((i[::-1]) ** 2)
    columns = [np.asarray(c, np.int32) for c in columns]
    want = [brute_column(g) for g in columns]
    ties = 0
    for g, (value, who) in zip(columns, want):                          # the patterns do tie: the rule decides something
        gg = np.where(g == FAR, np.int64(1) << 60, g.astype(np.int64))
        f = gg[None, :] + (np.arange(len(g))[:, None] - np.arange(len(g))[None, :]) ** 2
        ties += int((((f == f.min(axis=1, keepdims=True)).sum(axis=1) >= 2) & (value != FAR)).sum())
    assert ties > 300
    for stride, ring in ((1, 16), (3, 1), (1, 1), (3, 16)):
        got = host_scan(driver, tmp_path, columns, stride, ring)
        for g, (value, who), (ref_value, ref_who) in zip(columns, got, want):
            assert np.array_equal(value, ref_value), (len(g), stride, ring, g[:8])
            assert np.array_equal(who, ref_who), (len(g), stride, ring, g[:8], who[:8], ref_who[:8])


def test_the_row_function_names_the_left_source_at_a_tie(driver):
    rng = np.random.default_rng(6)
    cases = []
    for head in (0, 1, 2, 3):
        for n in (1, 2, 5, 31, 32, 33, 64, 65, 100):
            for p in (0.0, 0.03, 0.3, 1.0):
                cases.append((n, head, rng.random(n) < p))
            for ends in ((0,), (n - 1,), (0, n - 1)):                   # the row's two ends
                bits = np.zeros(n, bool)
                bits[list(ends)] = True
                cases.append((n, head, bits))
        # equidistant left and right, and across the word boundary between elements 31 and 32
        for left, right in ((2, 8), (0, 6), (31 - head, 35 - head), (30 - head, 34 - head), (28 - head, 36 - head), (10, 60)):
            bits = np.zeros(70, bool)
            bits[[left, right]] = True
            cases.append((70, head, bits))
    text = "".join(f"{n} {head} {''.join('1' if b else '0' for b in bits)}\n" for n, head, bits in cases)
    out = subprocess.run([driver, "rows"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(cases)
    ties = 0
    for (n, head, bits), line in zip(cases, out):
        d2, index = brute_force(bits.reshape(1, 1, -1))
        ties += int(tied(bits.reshape(1, 1, -1)).sum())
        want = [f"{int(d)}:{int(i)}" for d, i in zip(d2.reshape(-1), index.reshape(-1))]
        assert line.split() == want, (n, head, bits.astype(int))
    assert ties > 20


def plans(exe, cases):
    out = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    res = [line if line in ("empty", "extent", "voxels") else [int(v) for v in line.split()] for line in lines[1:]]
    assert len(res) == len(cases)
    return [int(v) for v in lines[0].split()], res


def test_nearest_plan_and_its_refusals(driver):
    cases = [(nx, 3, 2, h) for nx in (1, 3, 4, 5, 33, 65) for h in (0, 1, 3)] + [(7, 5, 3, 2), (1, 1, 1, 0), (1 << 10, 1 << 10, 1 << 10, 0), (MAX_EXTENT, MAX_EXTENT, 4, 3)]
    (no_owner, max_extent), res = plans(driver, cases)
    assert no_owner == NO_OWNER and max_extent == MAX_EXTENT <= NO_OWNER          # every owner fits 16 bits and misses the mark
    up = lambda v: -(-v // 16) * 16
    for (nx, ny, nz, head), (voxels, dist_bytes, ox, oy, oz, total) in zip(cases, res):
        assert voxels == nx * ny * nz
        # three planes of 2 bytes per voxel behind svr_distance's scratch, each at a multiple of 16
        assert ox == up(dist_bytes) and oy == ox + up(2 * voxels) and oz == oy + up(2 * voxels) and total == oz + up(2 * voxels) >= dist_bytes + 6 * voxels
    _, res = plans(driver, [(0, 4, 4, 0), (4, -1, 4, 0), (MAX_EXTENT + 1, 1, 1, 0), (1, 1, MAX_EXTENT + 1, 0), ((1 << 10) + 1, 1 << 10, 1 << 10, 0)])
    assert res == ["empty", "empty", "extent", "extent", "voxels"]


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_nearest" in N.SIGNATURES
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert "NearestField" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "nearest") and hasattr(SubVolume, "expand_labels")
    assert hasattr(C.CDLL(N.LIB_PATH), "svr_nearest")
    assert [f for f, _ in N.NearestParams._fields_] == [f for f, _ in N.DistanceParams._fields_ if f != "border"]


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    params = ["lod", "use_box", "box_off", "box_shape", "mode", "level", "selected", "selected_count", "ignore_zero", "invert"]
    outputs = ["d2", "index", "label", "capacity", "header"]
    fields = [f"offsetof(svr_nearest_params, {f})" for f in params] + [f"offsetof(svr_nearest_outputs, {f})" for f in outputs]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { size_t v[] = {sizeof(svr_nearest_params), '
                   "sizeof(svr_nearest_outputs), " + ", ".join(fields) + "}; for (size_t i = 0; i < sizeof v / sizeof *v; ++i) "
                   'printf("%zu ", v[i]); return 0; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.NearestParams), C.sizeof(N.NearestOutputs)] + [getattr(N.NearestParams, f).offset for f in params] + \
        [getattr(N.NearestOutputs, f).offset for f in outputs]
    assert got[:2] == [64, 40]                                          # 60 bytes of fields, padded to the pointer's alignment


def test_argument_errors_fire_without_a_gpu():
    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    for kw in (dict(level=0.5, labels=[1]), dict(invert=1), dict(with_labels=None), dict(background="yes"), dict(labels=[]), dict(labels="12"),
               dict(labels=[-1]), dict(labels=[1.5]), dict(level=float("nan")), dict(level="high"), dict(level=True), dict(lod=1), dict(level=1.0, lod=-1),
               dict(level=1.0, box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4)))):
        with pytest.raises(ValueError):
            vol.nearest(**kw)
    for kw in (dict(r=-1), dict(r="2"), dict(r=float("nan")), dict(r=True), dict(r=1, labels=[]), dict(r=1, lod=3)):
        with pytest.raises(ValueError):
            vol.expand_labels(**kw)
    assert nearest_arguments(None, None, False, False, True) == (N.COMPONENTS_LABELS, None, 0.0, 1, 0, True)
    mode, ids, level, ignore_zero, invert, with_labels = nearest_arguments(None, [3, 1, 3], True, True, False)
    assert (mode, ids.tolist(), ignore_zero, invert, with_labels) == (N.COMPONENTS_LABELS, [1, 3], 0, 1, False)
    assert nearest_arguments(7, None, False, True, True) == (N.COMPONENTS_LEVEL, None, 7.0, 0, 1, True)


def test_nearest_field_answers_on_the_cpu():
    """NearestField's methods are numpy and torch ops: on CPU tensors they answer from the twin's arrays."""
    import torch

    class World:
        matrix = np.diag([2.0, 1.0, 0.5, 1.0])

    class Volume:
        world = World()

    Volume.world.matrix[:3, 3] = (3.0, -2.0, 7.0)
    rng = np.random.default_rng(15)
    labels = np.zeros((6, 7, 8), np.uint32)
    labels[1:3, 1:3, 1:4] = 5
    labels[4, 5, 6] = 0xFFFFFFF0
    labels[0, 6, 7] = 2
    density = rng.random((6, 7, 8)).astype(np.float32)
    off, box = (16, 8, 40), ((17, 8, 41), (6, 7, 4))
    twin = nearest_twin(off, density, labels, box=box, ignore_zero=True, invert=True)
    head = twin["header"]
    nz, ny, nx = twin["d2"].shape
    assert (nz, ny, nx) == (4, 7, 6) and head[15] == 0

    def field(t, **kw):
        return NearestField(squared=torch.from_numpy(t["d2"].copy()), begin=(41, 8, 17), offset=off[::-1], inside_voxels=t["header"][1],
                            targets=t["header"][0], far_voxels=t["header"][15], max_squared=t["header"][3], deepest=(41, 8, 17), lod=1,
                            scale_factor=(0.5, 0.5, 0.25), volume=Volume(), index=torch.from_numpy(t["index"].copy()),
                            label=torch.from_numpy(t["label"].copy()), **kw)

    f = field(twin)
    i = twin["index"].astype(np.int64)
    want = np.stack([i // (ny * nx) + 41, i // nx % ny + 8, i % nx + 17], -1)
    assert np.array_equal(f.nearest_voxel().numpy(), want) and f.nearest_voxel().dtype == torch.int32
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vec = f.vector().numpy().astype(np.int64)
    assert np.array_equal(vec, want - np.stack([z + 41, y + 8, x + 17], -1)) and np.array_equal((vec ** 2).sum(-1), twin["d2"])
    for r in (0, 1, 1.5, np.sqrt(2.0), 2, 2.9, 100):
        got = f.expanded(r)
        assert got.dtype == torch.uint32 and np.array_equal(got.numpy(), expanded(twin, r)), r
        assert np.array_equal(got.numpy(), np.where(twin["d2"] <= r * r, twin["label"], 0))
    cut = labels[1:5, :, 1:7]
    assert np.array_equal(f.expanded(0).numpy(), cut)                   # r = 0: the objects themselves
    assert (f.expanded(100).numpy() != 0).all() and (f.expanded(100).numpy() == 0xFFFFFFF0).any()
    assert int((f.expanded(1.5).numpy() != 0).sum()) > int((f.expanded(1).numpy() != 0).sum()) > int((cut != 0).sum())
    for bad in (-1, float("nan"), "2", True, None):
        with pytest.raises(ValueError):
            f.expanded(bad)
    bare = field(twin)
    bare.label = None
    with pytest.raises(ValueError):
        bare.expanded(1)
    # FAR targets: never in expanded(), -1 in nearest_voxel(), 0 in vector(), None from nearest_position()
    far = nearest_twin(off, density, labels, box=box, selected=[77], invert=True)
    assert (far["d2"] == FAR).all() and (far["index"] == -1).all() and far["header"][15] == far["d2"].size
    ff = field(far)
    assert not ff.expanded(1e9).numpy().any() and (ff.nearest_voxel().numpy() == -1).all() and not ff.vector().numpy().any()
    mixed = field(twin)
    mixed.squared[0, 0, 0], mixed.index[0, 0, 0] = FAR, -1
    mixed.label.view(torch.int32)[0, 0, 0] = 9
    assert int(mixed.expanded(1e9)[0, 0, 0]) == 0 and int((mixed.expanded(1e9) != 0).sum()) == twin["d2"].size - 1
    # a picked point snaps to the centre of its voxel's nearest source
    to_world = lambda c: ((np.asarray(c, np.float64) + 0.5) / np.array([0.25, 0.5, 0.5]) - 0.5) * np.array([2.0, 1.0, 0.5]) + np.array([3.0, -2.0, 7.0])
    for k in rng.integers(0, z.size, 40):
        c = np.array([x.flat[k] + 17 + 0.3, y.flat[k] + 8 - 0.4, z.flat[k] + 41 + 0.2])                # shader order
        got = f.nearest_position(to_world(c))
        assert np.allclose(got, to_world(want.reshape(-1, 3)[k][::-1]), rtol=0, atol=1e-12)
        assert f.at(got) == 0 and f.at(to_world(c)) == int(twin["d2"].flat[k])                            # a source lies there
    assert f.nearest_position((-1000.0, 0.0, 0.0)) is None and ff.nearest_position(to_world((18, 9, 42))) is None
    assert count_only(head) == head[:2] + [0, 0] + head[4:14] + [0, 0]
