"""svr_components without a GPU: the numpy restatement (tests/components_twin.py) held to scipy.ndimage.label, numbering
included; the union-find and the host plan (csrc/components_uf.h, csrc/components_plan.h) compiled on their own with the
host compiler and run on volumes this test writes, single-threaded and with 8 threads joining concurrently; the plan's
properties; and the pins of the new surface (the symbol, the struct sizes, the argument errors of
``SubVolume.components``)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from components_twin import RECORD, components_twin, label_components, neighbour_offsets
from odd_ring_scenes import plan_cases
from parent_plans import held_to_parent
from sub_volume_renderer_amd import ComponentLabels, SubVolume, SubVolumeMaterial, _native as N
from sub_volume_renderer_amd.components import components_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
STRUCTURE = {6: ndimage.generate_binary_structure(3, 1), 26: np.ones((3, 3, 3), bool)}


def serpentine(shape):
    """A one-voxel path that runs to and fro along x, stepping in y at the row ends and in z at the plane ends, in every
    second row and plane: one component under either connectivity, with the longest chains a box of this size has."""
    nz, ny, nx = shape
    inside = np.zeros(shape, bool)
    right = True
    for zi, z in enumerate(range(0, nz, 2)):
        rows = list(range(0, ny, 2))
        if zi % 2:
            rows = rows[::-1]
        for yi, y in enumerate(rows):
            inside[z, y, :] = True
            end = nx - 1 if right else 0
            if yi + 1 < len(rows):
                inside[z, min(y, rows[yi + 1]):max(y, rows[yi + 1]) + 1, end] = True
            elif z + 2 < nz:
                inside[z:z + 3, y, end] = True
            right = not right
    return inside


def volumes():
    rng = np.random.default_rng(21)
    shape = (9, 11, 14)
    noise = rng.random(shape)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return [("54 %", noise < 0.54), ("25 %", noise < 0.25), ("11 %", noise < 0.11), ("checkerboard", (x + y + z) % 2 == 0),
            ("serpentine", serpentine(shape)), ("all", np.ones(shape, bool)), ("none", np.zeros(shape, bool)),
            ("one row", rng.random((1, 1, 37)) < 0.6), ("one column", rng.random((23, 1, 1)) < 0.6)]


# ---- the twin against scipy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_twin_is_scipy_label_numbering_included(connectivity):
    assert len(neighbour_offsets(connectivity)) == connectivity
    for name, inside in volumes():
        want, count = ndimage.label(inside, structure=STRUCTURE[connectivity])
        ids, roots = label_components(inside, None, connectivity)
        assert len(roots) == count and np.array_equal(ids, want.astype(np.uint32)), (name, connectivity)
        # a root is the first voxel of its component in (z, y, x) order
        flat = ids.reshape(-1)
        assert np.array_equal(flat[roots], np.arange(1, count + 1)), name
        for k in range(min(count, 20)):
            assert np.flatnonzero(flat == k + 1)[0] == roots[k], name
        if name == "checkerboard":
            assert count == (int(inside.sum()) if connectivity == 6 else 1)
        if name in ("serpentine", "all"):
            assert count == 1
        if name == "none":
            assert count == 0 and not ids.any()


def by_label_with_scipy(labels, inside, connectivity):
    """scipy run per label, the components renumbered by their first voxels."""
    out = np.zeros(labels.shape, np.int64)
    firsts = []
    for v in np.unique(labels[inside]):
        got, count = ndimage.label(inside & (labels == v), structure=STRUCTURE[connectivity])
        for k in range(1, count + 1):
            firsts.append((int(np.flatnonzero(got.reshape(-1) == k)[0]), got == k))
    for number, (_, where) in enumerate(sorted(firsts, key=lambda f: f[0])):
        out[where] = number + 1
    return out.astype(np.uint32), len(firsts)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_twin_splits_by_label_as_scipy_per_label_does(connectivity):
    rng = np.random.default_rng(4)
    labels = np.array([0, 5, 6, 0xFFFFFFF0], np.uint32)[rng.integers(0, 4, (8, 9, 13))]
    for inside in (np.ones(labels.shape, bool), labels != 0, np.isin(labels, [5, 0xFFFFFFF0])):
        want, count = by_label_with_scipy(labels, inside, connectivity)
        ids, roots = label_components(inside, labels, connectivity)
        assert len(roots) == count > 10 and np.array_equal(ids, want)


def test_components_twin_header_records_and_boxes():
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 3, (6, 7, 8)).astype(np.uint32)
    density = rng.random((6, 7, 8)).astype(np.float32)
    off = (16, 8, 40)
    twin = components_twin(off, density, labels, level=0.6, connectivity=26)
    inside = density >= np.float32(0.6)
    want, count = ndimage.label(inside, structure=STRUCTURE[26])
    assert twin["header"] == [count, int(inside.sum()), inside.size, count, 16, 8, 40, 16, 8, 40, 8, 7, 6, 0, 0, 0]
    assert np.array_equal(twin["ids"], want) and twin["records"].dtype == RECORD and len(twin["records"]) == count
    for r in twin["records"]:
        z, y, x = np.nonzero(want == r["id"])
        assert r["voxels"] == len(z) and r["label"] == 0 and r["reserved"] == 0
        assert r["sum"].tolist() == [int(x.sum()), int(y.sum()), int(z.sum())]
        assert r["first"].tolist() == [x[0] + 16, y[0] + 8, z[0] + 40]
        assert r["lo"].tolist() == [x.min() + 16, y.min() + 8, z.min() + 40] and r["hi"].tolist() == [x.max() + 16, y.max() + 8, z.max() + 40]
    # the label modes: every label, a selection, label 0 left out, labels joined
    every = components_twin(off, density, labels)
    assert every["header"][1] == labels.size and every["header"][13] == 0 and set(every["records"]["label"].tolist()) == {0, 1, 2}
    no_zero = components_twin(off, density, labels, ignore_zero=True)
    assert no_zero["header"][13] == int((labels == 0).sum()) and no_zero["header"][1] == int((labels != 0).sum())
    picked = components_twin(off, density, labels, selected=[2, 9], ignore_zero=True)
    assert picked["header"][13] == 0 and picked["header"][1] == int((labels == 2).sum()) and set(picked["records"]["label"].tolist()) == {2}
    joined = components_twin(off, density, labels, selected=[1, 2], join_labels=True)
    assert np.array_equal(joined["ids"], ndimage.label(labels != 0)[0]) and joined["header"][0] < components_twin(off, density, labels, selected=[1, 2])["header"][0]
    # a box partly outside the window is cut at the window: nothing connects across its border
    part = components_twin(off, density, labels, box=((10, 10, 42), (9, 3, 100)), level=0.5)
    inner = density[2:, 2:5, :3] >= np.float32(0.5)
    assert part["header"][7:13] == [16, 10, 42, 3, 3, 4] and np.array_equal(part["ids"], ndimage.label(inner)[0])
    assert part["records"]["sum"][0].tolist() == [int(v.sum()) for v in (lambda z, y, x: (x, y + 2, z + 2))(*np.nonzero(part["ids"] == 1))]
    for empty in (components_twin(off, density, labels, box=((0, 0, 0), (5, 5, 5))), components_twin((3, 4, 5), None, None, level=1.0),
                  components_twin(off, density, labels, box=((17, 9, 41), (0, 2, 2)), level=0.1)):
        assert empty["header"][:4] == [0, 0, 0, 0] and empty["header"][7:] == [0] * 9 and empty["ids"].size == 0 and len(empty["records"]) == 0
    # without label rings every label reads 0
    assert components_twin(off, density, None)["header"][:2] == [1, density.size]
    assert components_twin(off, density, None, ignore_zero=True)["header"][:2] == [0, 0]
    assert components_twin(off, density, None, ignore_zero=True)["header"][13] == density.size


# ---- the union-find and the plan on the host -----------------------------------------------------------------------------
# "label FILE nx ny nz head connectivity keyed threads OUT": FILE holds nx ny nz bytes of inside(), then as many u32 keys;
# OUT receives parent[] after the flatten pass, then the numbers (0 outside), u32 each.
# "plan" reads "nx ny nz head" lines -> "voxels head upr units levels count[4] parent_off aux_off off[4] bytes", "empty" or "too_many".
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "components_plan.h"
#include "components_uf.h"

template <bool C26, bool KEYED>
static void merge(uint32_t* parent, const uint32_t* aux, const CompPlan& p, int threads) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=, &p]() {
            // a "workgroup" of kBoxScanBlock voxels at a time, dealt round robin, so that neighbours are joined by different threads
            for (uint32_t b = (uint32_t)t; b < p.scan.count[0]; b += (uint32_t)threads)
                for (uint32_t i = b * kBoxScanBlock; i < p.voxels && i < (b + 1) * kBoxScanBlock; ++i)
                    uf_merge_voxel<C26, KEYED>(parent, aux, i, p.n, p.head);
        });
    for (auto& th : pool) th.join();
}

static int label(int argc, char** argv) {
    if (argc != 11) return 2;
    int64_t n[3] = {atoll(argv[3]), atoll(argv[4]), atoll(argv[5])};
    const uint32_t head = (uint32_t)atoi(argv[6]);
    const int conn = atoi(argv[7]), keyed = atoi(argv[8]), threads = atoi(argv[9]);
    CompPlan p;
    if (!comp_plan(n, head, p)) return 3;
    std::vector<uint8_t> inside(p.voxels);
    std::vector<uint32_t> parent(p.voxels), aux(p.voxels);
    FILE* f = fopen(argv[2], "rb");
    if (!f || fread(inside.data(), 1, p.voxels, f) != p.voxels || fread(aux.data(), 4, p.voxels, f) != p.voxels) return 4;
    fclose(f);
    // the init pass: the voxels of a unit of 4 elements are linked where they connect
    for (uint32_t unit = 0; unit < p.units; ++unit) {
        const uint32_t row = unit / p.upr, w = unit - row * p.upr;
        const int32_t r0 = (int32_t)(4u * w) - (int32_t)head;
        uint32_t start = 0; bool prev = false;
        for (int j = 0; j < 4; ++j) {
            const int32_t r = r0 + j;
            if (r < 0 || r >= (int32_t)p.n[0]) { prev = false; continue; }
            const uint32_t i = row * p.n[0] + (uint32_t)r;
            if (inside[i]) {
                if (!(prev && (!keyed || aux[i] == aux[i - 1]))) start = i;
                parent[i] = start;
            } else parent[i] = kUfOutside;
            prev = inside[i] != 0;
        }
    }
    if (conn == 26) { if (keyed) merge<true, true>(parent.data(), aux.data(), p, threads); else merge<true, false>(parent.data(), aux.data(), p, threads); }
    else            { if (keyed) merge<false, true>(parent.data(), aux.data(), p, threads); else merge<false, false>(parent.data(), aux.data(), p, threads); }
    // flatten, and the roots of every block of voxels: level 0 of the scan
    const BoxScanPlan& s = p.scan;
    std::vector<std::vector<uint32_t>> lev(s.levels);
    for (int k = 0; k < s.levels; ++k) lev[k].assign(s.count[k], 0u);
    for (uint32_t i = 0; i < p.voxels; ++i) {
        if (parent[i] == kUfOutside) continue;
        const uint32_t r = uf_find(parent.data(), i);
        (void)uf_min(parent.data() + i, r);
        if (r == i) ++lev[0][i / kBoxScanBlock];
    }
    for (int k = 0; k + 1 < s.levels; ++k)
        for (uint32_t i = 0; i < s.count[k]; ++i) lev[k + 1][i / kBoxScanBlock] += lev[k][i];
    for (int k = s.levels - 1; k >= 0; --k) {                // exclusive prefixes inside a block, plus the block's from above
        uint32_t run = 0;
        for (uint32_t i = 0; i < s.count[k]; ++i) {
            if (i % kBoxScanBlock == 0) run = k + 1 < s.levels ? lev[k + 1][i / kBoxScanBlock] : 0u;
            const uint32_t v = lev[k][i];
            lev[k][i] = run; run += v;
        }
    }
    std::vector<uint32_t> ids(p.voxels, 0u);
    for (uint32_t b = 0; b < s.count[0]; ++b) {
        uint32_t rank = lev[0][b];
        for (uint32_t i = b * kBoxScanBlock; i < p.voxels && i < (b + 1) * kBoxScanBlock; ++i)
            if (parent[i] == i) aux[i] = rank++;
    }
    for (uint32_t i = 0; i < p.voxels; ++i) if (parent[i] != kUfOutside) ids[i] = aux[parent[i]] + 1u;
    FILE* o = fopen(argv[10], "wb");
    if (!o || fwrite(parent.data(), 4, p.voxels, o) != p.voxels || fwrite(ids.data(), 4, p.voxels, o) != p.voxels) return 5;
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "label")) return label(argc, argv);
    printf("%u %d %" PRIu64 " %u\n", kBoxScanBlock, kBoxScanMaxLevels, kCompMaxVoxels, kUfOutside);
    for (;;) {
        int64_t n[3]; uint32_t head;
        if (scanf("%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNu32, &n[0], &n[1], &n[2], &head) != 4) return 0;
        CompPlan p; bool too_many = false;
        if (!comp_plan(n, head, p, &too_many)) { printf(too_many ? "too_many\n" : "empty\n"); continue; }
        printf("%u %u %u %u %d %u %u %u %u %" PRIu64 " %" PRIu64, p.voxels, p.head, p.upr, p.units, (int)p.scan.levels, p.scan.count[0],
               p.scan.count[1], p.scan.count[2], p.scan.count[3], p.parent_off, p.aux_off);
        for (int k = 0; k < kBoxScanMaxLevels; ++k) printf(" %" PRIu64, p.scan.off[k]);
        printf(" %" PRIu64 "\n", p.bytes);
    }
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("components_host")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def host_label(exe, tmp_path, inside, key, head, connectivity, threads):
    nz, ny, nx = inside.shape
    src, out = tmp_path / "volume.bin", tmp_path / "labels.bin"
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(inside, np.uint8).tobytes())
        f.write(np.ascontiguousarray(np.zeros(inside.shape, np.uint32) if key is None else key, "<u4").tobytes())
    subprocess.run([exe, "label", str(src), str(nx), str(ny), str(nz), str(head), str(connectivity), str(int(key is not None)), str(threads),
                    str(out)], check=True, timeout=60)
    got = np.fromfile(out, "<u4")
    return got[:inside.size].reshape(inside.shape), got[inside.size:].reshape(inside.shape)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_host_labelling_gives_the_twins_roots_and_ranks(driver, tmp_path, connectivity):
    rng = np.random.default_rng(12)
    cases = [(name, inside, None) for name, inside in volumes()]
    big = (24, 20, 70)                                      # more voxels than one scan block squared would need levels for: 33600 > 256
    cases.append(("big 40 %", rng.random(big) < 0.4, None))
    cases.append(("big serpentine", serpentine(big), None))
    labels = np.array([0, 5, 6, 0xFFFFFFF0], np.uint32)[rng.integers(0, 4, big)]
    cases.append(("by label", np.ones(big, bool), labels))
    cases.append(("by label, no zeros", labels != 0, labels))
    for name, inside, key in cases:
        ids, roots = label_components(inside, key, connectivity)
        want_parent = np.where(inside, roots[np.maximum(ids.astype(np.int64) - 1, 0)] if len(roots) else 0, 0xFFFFFFFF).astype(np.uint32)
        for head in (0, 3) if inside.size < 5000 else (1,):
            for threads in (1, 8):
                parent, got = host_label(driver, tmp_path, inside, key, head, connectivity, threads)
                assert np.array_equal(parent, want_parent), (name, head, threads, "roots")
                assert np.array_equal(got, ids), (name, head, threads, "ranks")


def plans(exe, cases):
    out = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    res = []
    for line in lines[1:]:
        if line in ("empty", "too_many"):
            res.append(line)
            continue
        w = [int(v) for v in line.split()]
        res.append(dict(voxels=w[0], head=w[1], upr=w[2], units=w[3], levels=w[4], count=w[5:9], parent_off=w[9], aux_off=w[10], cnt_off=w[11:15],
                        bytes=w[15]))
    assert len(res) == len(cases)
    return [int(v) for v in lines[0].split()], res


def test_components_plan(driver):
    (block, max_levels, max_voxels, outside), _ = plans(driver, [])
    assert (block, max_levels, max_voxels, outside) == (256, 4, 1 << 30, 0xFFFFFFFF) and max_voxels == N.COMPONENTS_MAX_VOXELS
    assert outside >= max_voxels                            # the marker is no voxel's index, and every index fits u32
    cases = [(nx, 3, 2, h) for nx in (1, 3, 4, 5, 65) for h in (0, 1, 3)]
    cases += [(block, 1, 1, 0), (block + 1, 1, 1, 0), (block, block, 1, 2), (block, block, 1 + 1, 0), (16, block * block // 16, 1, 0),
              (16, block * block // 16 + 1, 1, 0), (1 << 10, 1 << 10, 1 << 10, 0)]
    # the windows and boxes of tests/test_gpu_odd_rings.py: head is the ring slot modulo 4 of the first voxel
    odd = [(*n, lo[0] % ring[0] & 3) for ring, off, lo, n in plan_cases()]
    assert {c[3] for c in odd} == {0, 1, 2, 3} and {1, 3, 63} <= {c[0] for c in odd}
    cases += odd
    _, res = plans(driver, cases)
    for c, p in zip(cases, res):
        nx, ny, nz, head = c
        voxels = nx * ny * nz
        count = [-(-voxels // block)]
        while count[-1] > block:
            count.append(-(-count[-1] // block))
        assert p["voxels"] == voxels and p["head"] == head and p["upr"] == -(-(nx + head) // 4) and p["units"] == p["upr"] * ny * nz, (c, p)
        assert p["units"] <= voxels and 4 * p["upr"] >= nx + head > 4 * (p["upr"] - 1)
        assert p["levels"] == len(count) <= 3 and p["count"][:len(count)] == count and not any(p["count"][len(count):]), (c, p)
        assert p["count"][p["levels"] - 1] <= block
        # the scratch: parent, aux, then the levels, back to back, 4-byte entries
        assert p["parent_off"] == 0 and p["aux_off"] == 4 * voxels
        at = 8 * voxels
        for k in range(max_levels):
            assert p["cnt_off"][k] == at
            at += 4 * p["count"][k]
        assert p["bytes"] == at
        # the fourth level, which 2^30 voxels never need, takes no bytes; and nothing moved
        assert p["count"][3] == 0 and p["cnt_off"][3] == p["bytes"]
        held_to_parent("components", c, [p["parent_off"], p["aux_off"], *p["cnt_off"][:3], p["bytes"]])
    by = {tuple(c): p for c, p in zip(cases, res)}
    assert by[(block, 1, 1, 0)]["levels"] == 1 and by[(block + 1, 1, 1, 0)]["count"] == [2, 0, 0, 0]
    assert by[(block, block, 1, 2)]["levels"] == 1 and by[(block, block, 2, 0)]["count"] == [2 * block, 2, 0, 0]
    assert by[(16, block * block // 16, 1, 0)]["levels"] == 1 and by[(16, block * block // 16 + 1, 1, 0)]["levels"] == 2
    assert by[(1 << 10, 1 << 10, 1 << 10, 0)]["count"] == [1 << 22, 1 << 14, 1 << 6, 0]    # the most voxels, and the most levels


def test_components_plan_refusals(driver):
    _, res = plans(driver, [(0, 4, 4, 0), (4, -1, 4, 0), ((1 << 10) + 1, 1 << 10, 1 << 10, 0), ((1 << 30) + 1, 1, 1, 0), (1 << 40, 1 << 40, 1 << 40, 0),
                            (1 << 30, 1, 1, 3)])
    assert res[0] == "empty" and res[1] == "empty" and res[2] == "too_many" and res[3] == "too_many" and res[4] == "too_many"
    assert res[5]["voxels"] == 1 << 30 and res[5]["upr"] == (1 << 28) + 1 and res[5]["bytes"] < 1 << 34
    held_to_parent("components", (1 << 30, 1, 1, 3), [res[5]["parent_off"], res[5]["aux_off"], *res[5]["cnt_off"][:3], res[5]["bytes"]])


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_components" in N.SIGNATURES
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert re.search(r"#define SVR_COMPONENTS_MAX_VOXELS \(1u << 30\)", header)
    assert (N.COMPONENTS_LABELS, N.COMPONENTS_LEVEL) == (0, 1)
    assert "ComponentLabels" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "components")
    import __graft_entry__ as g
    import inspect

    assert "components_kernels.hip" in g.HIP_SOURCES
    assert "components_plan.h" in inspect.getsource(g.build_hip) and "components_uf.h" in inspect.getsource(g.build_hip)


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(svr_components_params), sizeof(svr_component_record), sizeof(svr_components_outputs), "
                   "offsetof(svr_components_params, selected), offsetof(svr_components_params, connectivity), offsetof(svr_component_record, first), "
                   "offsetof(svr_component_record, hi), offsetof(svr_components_outputs, records), offsetof(svr_components_outputs, header)); return 0; }\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ComponentsParams), C.sizeof(N.ComponentRecord), C.sizeof(N.ComponentsOutputs), N.ComponentsParams.selected.offset,
                   N.ComponentsParams.connectivity.offset, N.ComponentRecord.first.offset, N.ComponentRecord.hi.offset,
                   N.ComponentsOutputs.records.offset, N.ComponentsOutputs.header.offset]
    assert got[:3] == [64, 80, 40] and got[1] == N.COMPONENT_RECORD_BYTES == RECORD.itemsize
    assert [RECORD.fields[k][1] for k in ("id", "label", "voxels", "sum", "first", "lo", "hi", "reserved")] == \
        [getattr(N.ComponentRecord, k).offset for k in ("id", "label", "voxels", "sum", "first", "lo", "hi", "reserved")]


def test_argument_errors_fire_without_a_gpu():
    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    for kw in (dict(level=0.5, labels=[1]), dict(connectivity=18), dict(connectivity=6.0), dict(connectivity=True), dict(labels=[]), dict(labels="12"),
               dict(labels=[-1]), dict(labels=[1.5]), dict(level=float("nan")), dict(level="high"), dict(level=True), dict(lod=1), dict(level=1.0, lod=-1),
               dict(level=1.0, box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4)))):
        with pytest.raises(ValueError):
            vol.components(**kw)
    assert components_arguments(None, None, False, False, 6) == (N.COMPONENTS_LABELS, None, 0.0, 1, 0, 6)
    mode, ids, level, ignore_zero, join, conn = components_arguments(None, [3, 1, 3], True, True, 26)
    assert (mode, ids.tolist(), ignore_zero, join, conn) == (N.COMPONENTS_LABELS, [1, 3], 0, 1, 26)
    assert components_arguments(7, None, False, True, 6) == (N.COMPONENTS_LEVEL, None, 7.0, 0, 0, 6)
    assert components_arguments(float("inf"), None, False, False, 6)[2] == float("inf")


def test_component_labels_answers_on_the_cpu():
    """ComponentLabels' methods are numpy and torch ops: on CPU tensors they answer from the twin's records."""
    import torch

    class World:
        matrix = np.diag([2.0, 1.0, 0.5, 1.0])

    class Volume:
        world = World()

    Volume.world.matrix[:3, 3] = (3.0, -2.0, 7.0)
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 3, (6, 7, 8)).astype(np.uint32)
    off = (16, 8, 40)
    twin = components_twin(off, None if False else np.zeros(labels.shape, np.float32), labels, box=((17, 8, 41), (6, 7, 4)), ignore_zero=True)
    r = twin["records"]
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
    table = ComponentLabels(ids=torch.from_numpy(twin["ids"].astype(np.int32)), count=len(r), begin=(41, 8, 17), offset=off[::-1],
                            inside_voxels=twin["header"][1], background=twin["header"][13], label=i64(r["label"]), voxels=i64(r["voxels"]),
                            first=i64(r["first"][:, ::-1]), lo=i64(r["lo"][:, ::-1]), end=i64(r["hi"][:, ::-1] + 1),
                            centroid=torch.from_numpy((np.array(off, np.float64) + r["sum"] / r["voxels"][:, None].astype(np.float64))[:, ::-1].copy()),
                            lod=1, scale_factor=(0.5, 0.5, 0.25), volume=Volume())
    assert len(table) == len(r) > 5
    order = sorted(range(len(r)), key=lambda k: (-int(r["voxels"][k]), k))
    assert table.largest() == [order[0] + 1] and table.largest(4) == [k + 1 for k in order[:4]] and table.largest(10 ** 6) == [k + 1 for k in order]
    for label in (1, 2):
        assert table.pieces(label) == [int(k) + 1 for k in np.nonzero(r["label"] == label)[0]] and len(table.pieces(label)) > 1
    assert table.pieces(0) == [] and table.pieces(77) == []
    big = table.largest()[0]
    assert np.array_equal(table.mask([big]).numpy(), twin["ids"] == big) and np.array_equal(table.mask(big).numpy(), twin["ids"] == big)
    assert np.array_equal(table.mask([1, 3]).numpy(), np.isin(twin["ids"], [1, 3])) and not table.mask([0]).any()
    lo, hi = r["lo"][big - 1][::-1], r["hi"][big - 1][::-1]
    assert table.box(big) == (tuple(int(v) for v in np.floor(lo / np.array([0.5, 0.5, 0.25]))),
                              tuple(int(v) for v in np.ceil((hi + 1) / np.array([0.5, 0.5, 0.25]))))
    centroid = (np.array(off, np.float64) + r["sum"][big - 1] / float(r["voxels"][big - 1]))              # shader order
    data = (centroid + 0.5) / np.array([0.25, 0.5, 0.5]) - 0.5
    assert np.allclose(table.position(big), data * np.array([2.0, 1.0, 0.5]) + np.array([3.0, -2.0, 7.0]), rtol=0, atol=1e-12)
    for bad in (0, len(r) + 1, True, 1.0):
        with pytest.raises(KeyError):
            table.box(bad)
    # id_at: the centre of every voxel of the box, and a point half a LOD voxel off it, give the voxel's number; outside gives 0
    z, y, x = np.meshgrid(*[np.arange(n) for n in twin["ids"].shape], indexing="ij")
    for dz, dy, dx in ((0.0, 0.0, 0.0), (0.4, -0.4, 0.4)):
        for k in rng.integers(0, z.size, 40):
            c = np.array([x.flat[k] + 17 + dx, y.flat[k] + 8 + dy, z.flat[k] + 41 + dz])                   # LOD coordinates, shader order
            world = ((c + 0.5) / np.array([0.25, 0.5, 0.5]) - 0.5) * np.array([2.0, 1.0, 0.5]) + np.array([3.0, -2.0, 7.0])
            assert table.id_at(world) == int(twin["ids"].flat[k])
    assert table.id_at((-1000.0, 0.0, 0.0)) == 0 and table.id_at((1e6, 1e6, 1e6)) == 0
