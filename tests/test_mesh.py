"""svr_mesh without a GPU: known answers of the numpy restatement (tests/mesh_twin.py) worked out by hand, the host plan
csrc/mesh_plan.h compiled on its own with the host compiler, and the pins of the new surface (the symbol, the ABI
version, the struct sizes, the argument errors of ``SubVolume.mesh``)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mesh_twin import EDGES, area_volume, mesh_twin, surface_nets
from parent_plans import held_to_parent
from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial, SurfaceMesh, _native as N
from sub_volume_renderer_amd.mesh import mesh_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
f32 = np.float32


def edge_counts(triangles):
    """{directed edge: uses} of a triangle list."""
    t = np.asarray(triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    keys, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(keys, counts)}


def closed_and_oriented(vertices, triangles):
    """Every undirected edge is used by an even number of triangles and every directed edge as often as its reverse; no
    triangle repeats a vertex; every vertex is used."""
    d = edge_counts(triangles)
    for (a, b), c in d.items():
        assert a != b
        assert d.get((b, a), 0) == c, (a, b)
    assert sorted(set(np.asarray(triangles).reshape(-1).tolist())) == list(range(len(vertices)))


def euler(vertices, triangles):
    """V - E + F with the quads' diagonals as edges (triangles are faces)."""
    und = {tuple(sorted(k)) for k in edge_counts(triangles)}
    return len(vertices) - len(und) + len(triangles)


# ---- known answers of the twin ----------------------------------------------------------------------------------------
def test_edge_order_is_the_headers():
    assert [(a, d0) for a, d0, _ in EDGES] == [
        (0, (0, 0, 0)), (0, (0, 1, 0)), (0, (0, 0, 1)), (0, (0, 1, 1)),
        (1, (0, 0, 0)), (1, (1, 0, 0)), (1, (0, 0, 1)), (1, (1, 0, 1)),
        (2, (0, 0, 0)), (2, (1, 0, 0)), (2, (0, 1, 0)), (2, (1, 1, 0))]
    assert all(sum(d1) - sum(d0) == 1 and d1[a] == 1 for a, d0, d1 in EDGES)


def test_one_voxel():
    """One inside voxel p: 8 vertices at p +- 1/6 on every axis in ascending cell order, 6 quads = 12 triangles, a cube of
    edge 1/3.  Coordinates stay below 8, where an f32 ulp is 4.8e-7: 1e-6 covers the sum of three terms and the division."""
    inside = np.zeros((3, 4, 5), bool)
    inside[1, 2, 3] = True                                  # p = (x, y, z) = (3, 2, 1)
    v, t = surface_nets(inside, rel0=(1, 2, 3))             # relative to the window offset p is (4, 4, 4)
    assert v.shape == (8, 3) and t.shape == (12, 3) and v.dtype == f32 and t.dtype == np.int32
    want = np.array([[4 + sx / 6.0, 4 + sy / 6.0, 4 + sz / 6.0] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])
    assert np.abs(v - want).max() <= 1e-6
    closed_and_oriented(v, t)
    area, vol = area_volume(v, t)
    assert abs(vol - (1.0 / 3.0) ** 3) < 1e-6 and abs(area - 6.0 / 9.0) < 1e-5
    assert euler(v, t) == 2


@pytest.mark.parametrize("shape", [(1, 1, 2), (2, 3, 4), (5, 1, 3), (4, 4, 4)])
def test_solid_block(shape):
    """A solid a x b x c block: flat faces half a voxel beyond the outer voxel centres, V - E + F = 2, outward normals."""
    c, b, a = shape                                         # numpy order
    inside = np.zeros((c + 2, b + 3, a + 4), bool)
    inside[1:1 + c, 2:2 + b, 3:3 + a] = True
    v, t = surface_nets(inside)
    lo, hi = np.array([3, 2, 1], f32), np.array([3 + a - 1, 2 + b - 1, 1 + c - 1], f32)
    # a cell strictly inside a face has 4 crossing edges, all along the face's axis at t = 0.5: its vertex lies on the flat
    # face, half a voxel beyond the outer voxel centres; the cells on the block's edges and corners are pulled inward
    for ax in range(3):
        others = [x for x in range(3) if x != ax]
        inner = int(np.prod([(a, b, c)[o] - 1 for o in others]))
        assert int(np.isclose(v[:, ax], lo[ax] - 0.5, atol=1e-6).sum()) == inner, ax
        assert int(np.isclose(v[:, ax], hi[ax] + 0.5, atol=1e-6).sum()) == inner, ax
        assert v[:, ax].min() >= lo[ax] - 0.5 - 1e-6 and v[:, ax].max() <= hi[ax] + 0.5 + 1e-6
    closed_and_oriented(v, t)
    assert euler(v, t) == 2
    assert len(v) == (a + 1) * (b + 1) * (c + 1) - max(a - 1, 0) * max(b - 1, 0) * max(c - 1, 0)
    assert len(t) == 2 * 2 * (a * b + b * c + a * c)
    area, vol = area_volume(v, t)
    assert 0 < vol < a * b * c and vol > a * b * c - 2.0 * (a * b + b * c + a * c) * 0.5


def test_vertex_and_quad_order():
    rng = np.random.default_rng(3)
    inside = rng.random((5, 6, 7)) < 0.4
    v, t = surface_nets(inside, rel0=(0, 0, 0))
    # vertices: ascending cell (z, y, x).  A vertex lies inside its cell: cell = floor(position) + 1 in cell indices
    cell = np.floor(v).astype(np.int64) + 1
    key = (cell[:, 2] * 100 + cell[:, 1]) * 100 + cell[:, 0]
    assert (np.diff(key) > 0).all()
    # quads: a quad's triangles are adjacent and share q0 and q2; its third corner (k2) is the cell of p; ascending p, then axis
    assert len(t) % 2 == 0
    q = t.reshape(-1, 2, 3)
    assert (q[:, 0, 0] == q[:, 1, 0]).all() and (q[:, 0, 2] == q[:, 1, 1]).all()
    p_key = key[q[:, 0, 2]]
    assert (np.diff(p_key) >= 0).all()
    # within one p the axes ascend: the axis is the one on which all four cells of the quad agree
    quad_cells = cell[np.stack([q[:, 0, 0], q[:, 0, 1], q[:, 0, 2], q[:, 1, 2]], axis=1)]      # [Q, 4, 3]
    same = (quad_cells == quad_cells[:, :1, :]).all(axis=1)
    assert (same.sum(axis=1) == 1).all()
    axis = same.argmax(axis=1)
    order = p_key * 3 + axis
    assert (np.diff(order) > 0).all()
    # orientation: the normal of a quad whose p is inside points along +axis
    pad = np.zeros((7, 8, 9), bool)
    pad[1:-1, 1:-1, 1:-1] = inside
    pc = cell[q[:, 0, 2]]
    inp = pad[pc[:, 2], pc[:, 1], pc[:, 0]]                 # cell index i has its first corner at padded voxel i
    a, b, c = v[q[:, 0, 0]].astype(np.float64), v[q[:, 0, 1]].astype(np.float64), v[q[:, 0, 2]].astype(np.float64)
    normal = np.cross(b - a, c - a)
    along = normal[np.arange(len(axis)), axis]
    assert ((along > 0) == inp).all() and (along != 0).all()


def test_touching_at_an_edge_or_a_corner_stays_closed():
    for second in ((2, 2, 1), (1, 2, 2), (2, 2, 2)):        # two edges, then the corner
        inside = np.zeros((4, 4, 4), bool)
        inside[1, 1, 1] = True
        inside[second[2], second[1], second[0]] = True
        v, t = surface_nets(inside)
        closed_and_oriented(v, t)
        assert area_volume(v, t)[1] > 0
        assert len(t) == 24                                 # no face is shared: 12 quads
        # the shared lattice edge or corner is where the surface is not a manifold: an undirected edge with 4 triangles
        # (edge contact), or none (corner contact, where the two cubes share one vertex)
        und = {}
        for (i, j), n in edge_counts(t).items():
            und[tuple(sorted((i, j)))] = und.get(tuple(sorted((i, j))), 0) + n
        assert set(und.values()) <= {2, 4} and (4 in und.values()) == (second != (2, 2, 2))
        assert len(v) == (15 if second == (2, 2, 2) else 14)


def random_mask_with_every_case():
    """A random 50 % mask of 12^3 in which all 254 mixed corner masks occur (a condition of the input: reseed until it holds)."""
    for seed in range(100):
        inside = np.random.default_rng(seed).random((12, 12, 12)) < 0.5
        pad = np.zeros((14, 14, 14), np.uint8)
        pad[1:-1, 1:-1, 1:-1] = inside
        code = np.zeros((13, 13, 13), np.int64)
        for d in range(8):
            code |= pad[(d >> 2):(d >> 2) + 13, ((d >> 1) & 1):((d >> 1) & 1) + 13, (d & 1):(d & 1) + 13].astype(np.int64) << d
        if set(np.unique(code).tolist()) >= set(range(1, 255)):
            return inside
    raise AssertionError("no seed below 100 gives all 254 cases")


def test_every_mixed_corner_mask():
    inside = random_mask_with_every_case()
    v, t = surface_nets(inside)
    closed_and_oriented(v, t)
    assert area_volume(v, t)[1] > 0
    # LABELS vertices lie on multiples of 1 / (2 k), k <= 12, inside their cell
    frac = v - np.floor(v)
    assert (frac >= 0).all() and (frac < 1).all()


@pytest.mark.parametrize("seed", range(4))
def test_any_mask_encloses_a_positive_volume(seed):
    rng = np.random.default_rng(100 + seed)
    inside = rng.random((6, 7, 8)) < (0.1, 0.3, 0.6, 0.95)[seed]
    assert inside.any()
    v, t = surface_nets(inside, rel0=(seed, 2 * seed, 0))
    closed_and_oriented(v, t)
    assert area_volume(v, t)[1] > 0


def test_level_on_a_linear_ramp():
    """v = 2 x + 3 y - z + 1 and a level that no voxel equals: every vertex lies on the plane within 1e-6 (relative to the
    gradient's scale), except those of the caps where the box cuts the half space."""
    z, y, x = np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij")
    values = (2.0 * x + 3.0 * y - z + 1.0).astype(f32)
    level = f32(17.25)
    v, t = surface_nets(values >= level, values=values, level=level)
    closed_and_oriented(v, t)
    plane = 2.0 * v[:, 0].astype(np.float64) + 3.0 * v[:, 1] - v[:, 2] + 1.0 - float(level)
    interior = ((v > 0) & (v < np.array([6, 7, 8]))).all(axis=1)       # cells with all corners in the box
    assert interior.sum() > 20
    assert np.abs(plane[interior]).max() / np.sqrt(14.0) <= 1e-6
    assert area_volume(v, t)[1] > 0


def test_special_values_and_box_faces_give_half():
    values = np.zeros((3, 3, 4), f32)
    values[1, 1, 1] = 10.0                                  # inside at level 4; neighbours 0, +x neighbour special
    for special in (np.nan, -np.inf):
        values[1, 1, 2] = special
        v, t = surface_nets(values >= f32(4.0), values=values, level=4.0)
        assert len(v) == 8
        # the x-edges toward the special value sit at 0.5, those toward 0 at (4 - 10) / (0 - 10) = 0.6 from the inside end
        assert np.isclose(v[:, 0].max(), 1.0 + (0.5 + 0.0 + 0.0) / 3.0, atol=1e-6)
        assert np.isclose(v[:, 0].min(), 0.0 + (0.4 + 1.0 + 1.0) / 3.0, atol=1e-6)
    values[1, 1, 2] = np.inf                                # inside, not finite: its edges to finite outside ends are at 0.5
    v, t = surface_nets(values >= f32(4.0), values=values, level=4.0)
    assert np.isclose(v[:, 0].max(), 2.0 + 0.5 / 3.0, atol=1e-6) and len(v) == 12
    # a voxel on the box's face: the edge that leaves the box is at 0.5, whatever the values
    edge = np.full((1, 1, 1), 10.0, f32)
    v, t = surface_nets(edge >= f32(4.0), values=edge, level=4.0)
    assert np.allclose(np.abs(v), 1.0 / 6.0, atol=1e-6)
    assert len(v) == 8 and len(t) == 12
    # v1 - v0 overflows to -inf: the quotient is 0, t = 0.  level - v0 overflows too: the quotient is NaN, t = 0.5.
    # The 4 cells on the far side of voxel 0 have the x-edge as their only crossing edge with a non-zero x: x = t / 3
    for v1, level, t_want in ((-3e38, 0.0, 0.0), (-3.4e38, -3e38, 0.5)):
        big = np.array([[[3e38, v1]]], f32)
        v, t = surface_nets(big >= f32(level), values=big, level=level)
        assert np.isfinite(v).all() and len(v) == 8 and np.isclose(v[:, 0].max(), t_want / 3.0, atol=1e-7)


def test_mesh_twin_boxes_and_header():
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 4, (6, 7, 8)).astype(np.uint32)
    density = rng.random((6, 7, 8)).astype(f32)
    off = (16, 8, 40)
    whole = mesh_twin(off, density, labels, selected=[1, 3])
    assert whole["header"][:4] == [len(whole["vertices"]), len(whole["triangles"])] * 2 and whole["header"][4:7] == list(off)
    assert whole["header"][7] == int(np.isin(labels, [1, 3]).sum())
    # a box partly outside the window is cut at the window; one that misses it is empty; so is a window of None
    part = mesh_twin(off, density, labels, box=((10, 10, 42), (9, 3, 100)), level=0.5)
    inner = density[2:, 2:5, :3]
    v, t = surface_nets(inner >= f32(0.5), rel0=(0, 2, 2), values=inner, level=0.5)
    assert np.array_equal(part["vertices"], v) and np.array_equal(part["triangles"], t) and part["header"][7] == int((inner >= 0.5).sum())
    for empty in (mesh_twin(off, density, labels, box=((0, 0, 0), (5, 5, 5)), selected=[1]), mesh_twin((0, 0, 0), None, None, level=1.0),
                  mesh_twin(off, density, labels, box=((17, 9, 41), (0, 2, 2)), selected=[1])):
        assert empty["header"][:4] == [0, 0, 0, 0] and empty["header"][7] == 0 and len(empty["vertices"]) == 0
    # without label rings every label reads 0
    solid = mesh_twin(off, density, None, selected=[0])
    assert solid["header"][7] == density.size and len(solid["triangles"]) == 4 * (6 * 7 + 7 * 8 + 6 * 8)
    assert mesh_twin(off, density, None, selected=[5])["header"][:4] == [0, 0, 0, 0]


# ---- the host plan ---------------------------------------------------------------------------------------------------
# per line "nx ny nz head" -> "cells[3] head bpr bit_words wpr rows words levels count[4] nib_off cnt_off[4] bit_off bytes", "empty" or "too_many"
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include "mesh_plan.h"
int main() {
    printf("%u %u %d %" PRIu64 "\n", kMeshCellsPerWord, kBoxScanBlock, kBoxScanMaxLevels, kMeshMaxCells);
    for (;;) {
        int64_t n[3]; uint32_t head;
        if (scanf("%" SCNd64 "%" SCNd64 "%" SCNd64 "%" SCNu32, &n[0], &n[1], &n[2], &head) != 4) return 0;
        MeshPlan p; bool too_many = false;
        if (!mesh_plan(n, head, p, &too_many)) { printf(too_many ? "too_many\n" : "empty\n"); continue; }
        printf("%u %u %u %u %u %u %u %u %u %d", p.cells[0], p.cells[1], p.cells[2], p.head, p.bpr, p.bit_words, p.wpr, p.rows, p.words, (int)p.scan.levels);
        for (int k = 0; k < kBoxScanMaxLevels; ++k) printf(" %u", p.scan.count[k]);
        printf(" %" PRIu64, p.nib_off);
        for (int k = 0; k < kBoxScanMaxLevels; ++k) printf(" %" PRIu64, p.scan.off[k]);
        printf(" %" PRIu64 " %" PRIu64 "\n", p.bit_off, p.bytes);
    }
}
"""


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("mesh_plan")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def plans(exe, cases):
    out = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    consts = [int(v) for v in lines[0].split()]
    res = []
    for line in lines[1:]:
        if line in ("empty", "too_many"):
            res.append(line)
            continue
        w = [int(v) for v in line.split()]
        res.append(dict(cells=w[0:3], head=w[3], bpr=w[4], bit_words=w[5], wpr=w[6], rows=w[7], words=w[8], levels=w[9], count=w[10:14],
                        nib_off=w[14], cnt_off=w[15:19], bit_off=w[19], bytes=w[20]))
    assert len(res) == len(cases)
    return consts, res


def expected_plan(n, head, per_word, block):
    cells = [v + 1 for v in n]
    wpr = -(-cells[0] // per_word)
    words = wpr * cells[1] * cells[2]
    count = [words]
    while count[-1] > block:
        count.append(-(-count[-1] // block))
    return cells, wpr, words, count


def test_mesh_plan(plan_driver):
    consts, _ = plans(plan_driver, [])
    per_word, block, max_levels, max_cells = consts
    assert (per_word, block, max_levels, max_cells) == (16, 256, 4, 1 << 28) and max_cells == N.MESH_MAX_CELLS
    cases = [(cx - 1, 3, 2, h) for cx in (15, 16, 17, 63, 64, 65) for h in (0, 3)]
    # a word count just above one scan block, and just above one block of block sums (rows of one word)
    cases += [(15, block, 0 + 1, 0), (15, block + 1 - 1, 1, 1), (15, block * block // 2, 1, 2), (15, block * block, 1, 0), (7, 2, 4, 1)]
    _, res = plans(plan_driver, cases)
    for c, p in zip(cases, res):
        n, head = list(c[:3]), c[3]
        cells, wpr, words, count = expected_plan(n, head, per_word, block)
        assert p["cells"] == cells and p["wpr"] == wpr and p["rows"] == cells[1] * cells[2] and p["words"] == words, (c, p)
        assert p["levels"] == len(count) and p["count"][:len(count)] == count and not any(p["count"][len(count):]), (c, p)
        assert p["count"][p["levels"] - 1] <= block
        assert p["head"] == head and p["bpr"] == -(-(n[0] + head) // 32) and p["bit_words"] == p["bpr"] * n[1] * n[2]
        # the scratch: the words of cells, the levels, the bits, back to back, 8-byte entries
        at = 0
        assert p["nib_off"] == at
        at += 8 * words
        for k in range(max_levels):
            assert p["cnt_off"][k] == at
            at += 8 * p["count"][k]
        assert p["bit_off"] == at and p["bytes"] == at + 4 * p["bit_words"]
        held_to_parent("mesh", c, [p["nib_off"], *p["cnt_off"], p["bit_off"], p["bytes"]])
        cells_n = cells[0] * cells[1] * cells[2]
        assert p["bytes"] <= 16 * words + 8 * sum(p["count"][1:]) + 4 * p["bit_words"]
        assert wpr * per_word >= cells[0] > (wpr - 1) * per_word and words <= cells_n
    by = {tuple(c): p for c, p in zip(cases, res)}
    assert [by[(cx - 1, 3, 2, 0)]["wpr"] for cx in (15, 16, 17, 63, 64, 65)] == [1, 1, 2, 4, 4, 5]
    assert by[(15, block, 1, 0)]["words"] == 2 * (block + 1) and by[(15, block, 1, 0)]["levels"] == 2
    assert by[(15, block, 1, 1)]["count"][:2] == [2 * (block + 1), 3]
    assert by[(15, block * block // 2, 1, 2)]["words"] == block * block + 2 and by[(15, block * block // 2, 1, 2)]["levels"] == 3
    assert by[(15, block * block // 2, 1, 2)]["count"][:3] == [block * block + 2, block + 1, 2]
    assert by[(15, block * block, 1, 0)]["levels"] == 3


def test_mesh_plan_refusals(plan_driver):
    _, res = plans(plan_driver, [(0, 4, 4, 0), (4, -1, 4, 0), (1 << 14, 1 << 14, 1, 0), ((1 << 28) - 1, 0 + 1, 0 + 1, 0),
                                 (1 << 28, 1, 1, 0), (1, (1 << 13) - 1, (1 << 14) - 1, 0), (1 << 40, 1 << 40, 1 << 40, 0)])
    assert res[0] == "empty" and res[1] == "empty"
    assert res[2] == "too_many"                             # (2^14 + 1)^2 * 2 cells
    assert res[3] == "too_many"                             # 2^28 * 2 * 2
    assert res[4] == "too_many" and res[6] == "too_many"
    # exactly 2^28 cells in rows of one word: the most words there can be, and the most levels
    assert res[5]["cells"] == [2, 1 << 13, 1 << 14] and res[5]["levels"] == 4 and res[5]["count"] == [1 << 27, 1 << 19, 1 << 11, 1 << 3]
    held_to_parent("mesh", (1, (1 << 13) - 1, (1 << 14) - 1, 0), [res[5]["nib_off"], *res[5]["cnt_off"], res[5]["bit_off"], res[5]["bytes"]])


# ---- the surface ---------------------------------------------------------------------------------------------------------
def test_surface_pins():
    assert "svr_mesh" in N.SIGNATURES
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", header).group(1)) == 9
    assert re.search(r"#define SVR_MESH_MAX_CELLS \(1u << 28\)", header)
    assert (N.MESH_LABELS, N.MESH_LEVEL) == (0, 1)
    assert "SurfaceMesh" in __import__("sub_volume_renderer_amd").__all__ and hasattr(SubVolume, "mesh")
    import __graft_entry__ as g
    import inspect

    assert "mesh_kernels.hip" in g.HIP_SOURCES and "mesh_plan.h" in inspect.getsource(g.build_hip)


def test_struct_sizes_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(svr_mesh_params), sizeof(svr_mesh_outputs), offsetof(svr_mesh_params, mode), offsetof(svr_mesh_params, selected), "
                   "offsetof(svr_mesh_outputs, header), offsetof(svr_mesh_outputs, triangle_capacity)); return 0; }\n")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.MeshParams), C.sizeof(N.MeshOutputs), N.MeshParams.mode.offset, N.MeshParams.selected.offset,
                   N.MeshOutputs.header.offset, N.MeshOutputs.triangle_capacity.offset]
    assert got[:2] == [56, 40]


def test_argument_errors_fire_without_a_gpu():
    pairs = [(np.zeros((16, 16, 16), np.uint8), np.zeros((16, 16, 16), np.uint32))]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs, (2, 2, 2), (8, 8, 8))
    for kw in (dict(), dict(labels=[1], level=0.5), dict(labels=[]), dict(labels="12"), dict(labels=[-1]), dict(labels=[1.5]),
               dict(level=float("nan")), dict(level="high"), dict(level=True), dict(labels=[1], lod=1), dict(level=1.0, lod=-1),
               dict(level=1.0, box=((0, 0, 0),)), dict(labels=[1], box=((0, 0, 0), (0, 4, 4)))):
        with pytest.raises(ValueError):
            vol.mesh(**kw)
    assert mesh_arguments([3, 1, 3], None)[1].tolist() == [1, 3] and mesh_arguments(None, 7)[::2] == (N.MESH_LEVEL, 7.0)
    assert mesh_arguments(None, float("inf"))[2] == float("inf")


def test_surface_mesh_measures_on_the_cpu(tmp_path):
    """SurfaceMesh's methods are torch ops: on CPU tensors they give the twin's f64 numbers (the GPU test repeats this on the device)."""
    import torch

    inside = np.zeros((5, 6, 7), bool)
    inside[1:4, 2:5, 1:6] = True
    v, t = surface_nets(inside, rel0=(2, 0, 1))
    m = SurfaceMesh(torch.from_numpy(v), torch.from_numpy(t), offset=(8, 16, 24), inside_voxels=int(inside.sum()), lod=1,
                    scale_factor=(0.5, 0.5, 0.25))
    from sub_volume_renderer_amd._wobject import lod_center_to_data

    want = lod_center_to_data(v.astype(np.float64) + np.array([8.0, 16.0, 24.0]), (0.25, 0.5, 0.5))       # shader order
    assert np.array_equal(m.data_vertices().numpy(), want) and np.array_equal(m.world_vertices().numpy(), want)
    area, vol = area_volume(want, t)
    assert abs(m.area() - area) <= 1e-9 * area and abs(m.enclosed_volume() - vol) <= 1e-9 * vol and vol > 0
    path = tmp_path / "m.obj"
    m.write_obj(path)
    lines = open(path).read().split("\n")
    vs = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])
    fs = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("f ")])
    assert np.array_equal(vs, want) and np.array_equal(fs - 1, t)
