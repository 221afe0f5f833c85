"""CPU: the numpy restatement of svr_objects (tests/objects_twin.py) against a triple-loop brute force on a small wrapped
ring, the pure helpers behind ``ObjectTable.box`` and ``ObjectTable.position``, the argument checks of
``SubVolume.objects`` that need no device, and the ctypes mirrors of the new structs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from objects_twin import RECORD, box_twin, brute_force, objects_twin, position_twin
from sub_volume_renderer_amd import ObjectTable, SubVolume, SubVolumeMaterial, _native as N, _wobject as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_ring(labels=True):
    """A 6 x 5 x 4 ring (x, y, z) whose window (5 x 4 x 3 from (4, 3, 2)) wraps on every axis."""
    rng = np.random.default_rng(5)
    density = rng.integers(0, 256, (4, 5, 6), dtype=np.uint8)
    lab = rng.choice(np.array([0, 0, 1, 7, 0xFFFFFFFF, 2**31 + 3], np.uint32), (4, 5, 6)) if labels else None
    return dict(density=density, labels=lab, offset=(4, 3, 2), shape=(5, 4, 3), scale=(1.0, 1.0, 1.0))


@pytest.mark.parametrize("box", [None, ((5, 3, 3), (3, 9, 1)), ((0, 0, 0), (3, 3, 3)), ((6, 5, 4), (1, 1, 1))])
@pytest.mark.parametrize("labels", [None, [7], [0, 0xFFFFFFFF, 12345]])
@pytest.mark.parametrize("ignore_zero", [False, True])
def test_twin_equals_the_triple_loop(box, labels, ignore_zero):
    ring = small_ring()
    twin, brute = objects_twin(ring, box, labels, ignore_zero), brute_force(ring, box, labels, ignore_zero)
    assert twin["header"] == brute["header"]
    assert sorted(twin["objects"]) == sorted(brute["objects"])
    for label, rec in brute["objects"].items():
        got = twin["objects"][label]
        for k in ("voxels", "finite", "value_sum"):
            assert got[k] == rec[k], (label, k)
        for k in ("sum", "lo", "hi"):
            assert tuple(got[k]) == tuple(rec[k]), (label, k)
        assert (got["vmin"], got["vmax"]) == (float(rec["vmin"]), float(rec["vmax"]))
    if box is None and labels is None:
        assert twin["header"][1] + twin["header"][3] == 5 * 4 * 3 and len(twin["objects"]) >= 4
        assert (twin["header"][3] > 0) == ignore_zero and (0 in twin["objects"]) != ignore_zero
    if box == ((0, 0, 0), (3, 3, 3)):
        assert twin["header"][:4] == [0, 0, 0, 0]                    # the box misses the window


def test_twin_without_label_rings_and_on_float_values():
    ring = small_ring(labels=False)
    twin = objects_twin(ring)
    assert list(twin["objects"]) == [0] and twin["objects"][0]["voxels"] == 60
    assert twin["objects"][0]["lo"] == (4, 3, 2) and twin["objects"][0]["hi"] == (8, 6, 4)
    assert objects_twin(ring, ignore_zero=True)["header"][:4] == [0, 0, 0, 60]
    ring["density"] = ring["density"].astype(np.float32) - np.float32(100.0)
    ring["density"][0, 0, 0], ring["density"][3, 4, 5], ring["density"][2, 3, 4] = np.nan, np.inf, -np.inf   # slots (0,0,0), (5,4,3), (4,3,2)
    rec = objects_twin(ring)["objects"][0]
    assert rec["voxels"] == 60 and rec["finite"] == 57 and np.isfinite([rec["value_sum"], rec["vmin"], rec["vmax"]]).all()
    assert rec["abs_sum"] >= abs(rec["value_sum"])


def test_inverse_box_and_centroid_mapping():
    # finest_box is the inverse of lod_box: a LOD box comes back from the round trip
    for scale in ((1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (0.25, 0.5, 1.0)):
        for begin, end in (((0, 0, 0), (1, 1, 1)), ((3, 7, 2), (9, 8, 31)), ((-4, 0, 5), (-1, 6, 6))):
            fb, fe = W.finest_box(begin, end, scale)
            assert all(isinstance(v, int) for v in fb + fe)
            assert W.lod_box(fb, fe, scale) == (begin, end)
            assert (fb, fe) == box_twin(begin[::-1], tuple(v - 1 for v in end[::-1]), scale)
    assert W.finest_box((3, 7, 2), (9, 8, 31), (0.5, 0.5, 0.5)) == ((6, 14, 4), (18, 16, 62))
    # a LOD voxel's centre: voxel 0 of a half-scale LOD covers finest voxels 0 and 1, whose centres are 0 and 1
    assert W.lod_center_to_data(0.0, 0.5) == 0.5 and W.lod_center_to_data(3.0, 1.0) == 3.0
    assert np.array_equal(W.lod_center_to_data([1.5, 0.0, 2.0], [0.25, 0.5, 1.0]), [7.5, 0.5, 2.0])
    # the borders of the voxel map to the borders of the finest voxels it covers: [c - 0.5, c + 0.5) -> [c / s - 0.5, (c + 1) / s - 0.5)
    assert W.lod_center_to_data(2.0 - 0.5, 0.5) == 2.0 / 0.5 - 0.5 and W.lod_center_to_data(2.0 + 0.5, 0.5) == 3.0 / 0.5 - 0.5


def test_position_twin_goes_through_the_world_matrix():
    rec = dict(voxels=4, sum=(6, 2, 10))
    world = [[2.0, 0, 0, 10.0], [0, 1.0, 0, -3.0], [0, 0, 0.5, 0.0], [0, 0, 0, 1.0]]
    # centroid (x, y, z) = (5 + 1.5, 7 + 0.5, 1 + 2.5) in LOD voxels at scale 0.5 -> data (13.5, 15.5, 7.5)
    assert position_twin(rec, (5, 7, 1), (0.5, 0.5, 0.5), world) == (37.0, 12.5, 3.75)


def pairs(n=3, base=32):
    return [(np.zeros((base >> k, base >> k, 2 * (base >> k)), np.uint8), np.zeros((base >> k, base >> k, 2 * (base >> k)), np.uint32))
            for k in range(n)]


def test_argument_checks_need_no_device():
    assert W._OBJECTS_FIRST_CAPACITY == 4096
    assert W.objects_capacity(None) == (4096, True) and W.objects_capacity(None, 3) == (3, True)
    assert W.objects_capacity(1) == (1, False) and W.objects_capacity(np.int64(1 << 26), 5) == (1 << 26, False)
    for bad in (0, -1, (1 << 26) + 1, 4096.0, "4096", True):
        with pytest.raises(ValueError):
            W.objects_capacity(bad)
    assert W.label_ids([7, 3, 7, 0xFFFFFFFF, 0]).tolist() == [0, 3, 7, 0xFFFFFFFF]
    vol = SubVolume(SubVolumeMaterial(0.5), pairs(), [(2, 2, 2), (3, 3, 3), (4, 4, 4)], [(8, 8, 8), (4, 4, 4), (2, 2, 2)])
    for kw in (dict(lod=3), dict(lod=-1), dict(lod=True), dict(capacity=0), dict(capacity=2.5), dict(capacity=(1 << 26) + 1),
               dict(labels=[]), dict(labels=[-1]), dict(labels=[2**32]), dict(labels="12"), dict(labels=[1.5]),
               dict(box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4))), dict(box=((0, 0, 0), (4, 4, float("nan"))))):
        with pytest.raises(ValueError):
            vol.objects(**kw)


def test_object_table_lookups_on_host_tensors():
    import torch

    class World:
        matrix = np.diag([2.0, 2.0, 2.0, 1.0])

    class Volume:
        world = World()

    table = ObjectTable(ids=torch.tensor([0, 9, 0xFFFFFFFF]), voxels=torch.tensor([5, 2, 1]),
                        begin=torch.tensor([[0, 0, 0], [3, 2, 1], [7, 7, 7]]), end=torch.tensor([[4, 4, 4], [5, 3, 4], [8, 8, 8]]),
                        centroid=torch.tensor([[1.0, 1.0, 1.0], [3.5, 2.0, 2.0], [7.0, 7.0, 7.0]], dtype=torch.float64),
                        finite=torch.tensor([5, 2, 1]), mean=torch.zeros(3, dtype=torch.float64), min=torch.zeros(3), max=torch.zeros(3),
                        considered=8, background=0, lod=1, scale_factor=(0.5, 0.5, 0.5), volume=Volume())
    assert len(table) == 3 and table.index(9) == 1 and table.index(0xFFFFFFFF) == 2
    for absent in (1, 10, 2**32):
        with pytest.raises(KeyError):
            table.index(absent)
    assert table.box(9) == ((6, 4, 2), (10, 6, 8))
    # centroid (z, y, x) = (3.5, 2, 2) at scale 0.5 -> data (x, y, z) = (4.5, 4.5, 7.5) -> world * 2
    assert table.position(9) == (9.0, 9.0, 15.0)


def test_struct_mirrors_match_the_header(tmp_path):
    assert C.sizeof(N.ObjectRecord) == N.OBJECT_RECORD_BYTES == RECORD.itemsize == 96
    assert C.sizeof(N.ObjectsParams) == 56 and C.sizeof(N.ObjectsOutputs) == 16
    for name, _ in N.ObjectRecord._fields_:
        assert getattr(N.ObjectRecord, name).offset == RECORD.fields[name][1], name
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert "#define SVR_OBJECTS_MAX_CAPACITY (1u << 26)" in header and N.OBJECTS_MAX_CAPACITY == 1 << 26
    assert "svr_objects" in N.SIGNATURES
    gcc = shutil.which("gcc")
    if gcc is None:
        return                                                          # the ctypes sizes above still hold the layout
    unit = tmp_path / "sizes.c"
    unit.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                    "sizeof(svr_objects_params), sizeof(svr_object_record), sizeof(svr_objects_outputs), "
                    "offsetof(svr_objects_params, selected), offsetof(svr_objects_params, capacity), offsetof(svr_object_record, vmin)); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(unit), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [56, 96, 16, N.ObjectsParams.selected.offset, N.ObjectsParams.capacity.offset, N.ObjectRecord.vmin.offset]
