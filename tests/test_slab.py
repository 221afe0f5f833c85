"""Thick-slab projections without a GPU: the numpy restatement of svr_slab (tests/slab_twin.py) against reductions
over the SOURCE arrays, against slice_twin at N = 1, on partially resident slabs, ties and NaN, the depth plane;
every host-side refusal of SubVolume.render_slab; axis_slab_plane; and the C entry point in header, binding and
library."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import lmip
from slab_twin import slab_twin, twin_of_spec, w_len_of
from slice_twin import DISCARD, HIT, MISS, material_of
from slice_twin import twin_of_spec as slice_of_spec
from sub_volume_renderer_amd import FrameRegion, SliceResult, SubVolume, SubVolumeMaterial, _native
from test_slice import moved_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
Z, Y, X = (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)


def from_sources(spec, vol, xx, yy, z):
    """value / label / lod at the integer data-space voxels (xx, yy, z) from the source arrays (lod 255: none)."""
    value = np.zeros(xx.shape, np.float32)
    label = np.zeros(xx.shape, np.uint32)
    lod = np.full(xx.shape, 255, np.uint8)
    done = np.zeros(xx.shape, bool)
    for l, ((data, labels), b) in enumerate(zip(spec.pairs, vol.wrapping_buffers)):
        u = b.uniform()
        ic = [np.floor(d * np.float32(u["scale"][k])).astype(np.int64) for k, d in enumerate((xx, yy, np.full_like(xx, z)))]
        inb = ~done
        for k in range(3):
            inb &= (u["offset"][k] <= ic[k]) & (ic[k] < u["offset"][k] + u["shape"][k])
        value[inb] = data[ic[2][inb], ic[1][inb], ic[0][inb]]
        label[inb] = labels[ic[2][inb], ic[1][inb], ic[0][inb]]
        lod[inb] = l
        done |= inb
    return value, label, lod


@pytest.mark.parametrize("mode", ["max", "min", "mean"])
def test_z_slab_on_voxel_centres_reduces_the_source_voxels_after_wrapping_moves(mode):
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    assert any(int(o) % r for b in vol.wrapping_buffers for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1]))
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    for z, n in ((30, 7), (41, 5), (3, 9), (61, 7)):          # the last two reach past the box's faces
        out = twin_of_spec(spec, (31.5, 31.5, float(z)), X, Y, Z, n, mode, N, N, vol=vol)
        ks = [k for k in range(n) if 0 <= z + k - (n - 1) // 2 < N]
        per = [from_sources(spec, vol, xx, yy, z + k - (n - 1) // 2) for k in ks]
        vals = np.stack([p[0] for p in per])
        hit = np.stack([p[2] for p in per]) != 255
        anyhit = hit.any(0)
        pick = (np.where(hit, vals, -np.inf).argmax(0) if mode != "min" else np.where(hit, vals, np.inf).argmin(0))
        take = lambda a: np.take_along_axis(np.stack(a), pick[None], 0)[0]
        np.testing.assert_array_equal(out["flags"], np.where(anyhit, HIT, MISS))
        np.testing.assert_array_equal(out["lod"], np.where(anyhit, take([p[2] for p in per]), 255))
        np.testing.assert_array_equal(out["label"], np.where(anyhit, take([p[1] for p in per]), 0))
        if mode == "mean":
            expect = np.where(hit, vals, 0).sum(0) / np.maximum(hit.sum(0), 1)    # integers: exact in any order
            np.testing.assert_array_equal(out["value"], np.where(anyhit, expect, 0).astype(np.float32))
        else:
            np.testing.assert_array_equal(out["value"], np.where(anyhit, take([p[0] for p in per]), 0))
        depth = (np.array(ks)[pick] - (n - 1) / 2).astype(np.float32)
        np.testing.assert_array_equal(out["depth"], np.where(anyhit, depth, 0))
        assert anyhit.sum() > 1000


def test_one_sample_max_is_the_slice():
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    planes = [((31.5, 31.5, 30.0), X, Y, Z), ((30.2, 33.1, 29.7), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7), (0.3, -0.8, 0.2)),
              ((31.5, 31.5, -0.5), X, Y, (0.0, 0.0, 1e30)), ((20.0, 31.5, 31.5), Y, Z, (3.0, 0.0, 0.0))]
    q = np.array([0.2, -0.3, 0.4, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    rot = spec.world()
    rot.set_rotation_quaternion(q)
    rot.scale = (1.3, 0.8, 1.1)
    for world_inv in (None, rot.inverse_matrix):
        for o, u, v, w in planes:
            a = twin_of_spec(spec, o, u, v, w, 1, "max", 50, 38, vol=vol, world_inv=world_inv)
            b = slice_of_spec(spec, o, u, v, 50, 38, vol=vol, world_inv=world_inv)
            for k in b:
                np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def test_partially_resident_slabs_mean_over_hits_and_miss_versus_discard():
    spec = moved_spec(levels=1)                 # one level whose window is smaller than the volume
    vol = lmip.oracle_volume(spec)
    b = vol.wrapping_buffers[0].uniform()
    z_end = int(b["offset"][2] + b["shape"][2])                 # first z plane past the window
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    # 9 samples centred on the window's far face: 4 inside the window, 5 beyond it
    out = twin_of_spec(spec, (31.5, 31.5, float(z_end)), X, Y, Z, 9, "mean", N, N, vol=vol)
    per = [from_sources(spec, vol, xx, yy, z_end + k - 4) for k in range(9)]
    hit = np.stack([p[2] for p in per]) != 255
    assert hit[:4].any() and not hit[4:].any()
    anyhit = hit.any(0)
    vals = np.where(hit, np.stack([p[0] for p in per]), 0)
    np.testing.assert_array_equal(out["value"][anyhit], (vals.sum(0) / np.maximum(hit.sum(0), 1))[anyhit].astype(np.float32))
    assert (out["flags"][~anyhit] == MISS).all() and (~anyhit).sum() > 100    # inside the box, never resident
    np.testing.assert_array_equal(out["rgba"][~anyhit], np.tile([0, 0, 0, 1], (int((~anyhit).sum()), 1)))
    assert (out["lod"][~anyhit] == 255).all() and not out["value"][~anyhit].any() and not out["depth"][~anyhit].any()
    # a slab wholly outside the box is DISCARD; one that reaches into it only where nothing is resident is MISS
    out = twin_of_spec(spec, (31.5, 31.5, -10.0), X, Y, Z, 9, "max", 8, 8, vol=vol)
    assert (out["flags"] == DISCARD).all() and not out["rgba"].any()
    out = twin_of_spec(spec, (31.5, 31.5, -4.0), X, Y, Z, 9, "max", 8, 8, vol=vol)
    assert (out["flags"] == MISS).all()


def one_ring(column, labels=None):
    """A 1-LOD ring of 2 x 2 pixels whose z column holds ``column`` (float32) everywhere."""
    n = len(column)
    d = np.broadcast_to(np.asarray(column, np.float32)[:, None, None], (n, 2, 2)).copy()
    lab = np.broadcast_to(np.arange(n, dtype=np.uint32)[:, None, None] if labels is None else labels, (n, 2, 2)).copy()
    return [dict(density=d, labels=lab, offset=(0, 0, 0), shape=(2, 2, n), scale=(1.0, 1.0, 1.0))]


def run_column(column, mode, w=(0.0, 0.0, 1.0)):
    n = len(column)
    mat = material_of({})
    return slab_twin(one_ring(column), np.eye(4), (2, 2, n), (0.5, 0.5, (n - 1) / 2.0), X, Y, w, n, mode, 2, 2, mat)


def test_ties_keep_the_lowest_sample_and_nan_follows_the_strict_comparison():
    nan = np.float32(np.nan)
    cases = [  # column, mode, expected value, chosen k (= label)
        ([1, 3, 3, 2], "max", 3, 1), ([2, 1, 3, 1], "min", 1, 1), ([5, 5, 5], "max", 5, 0), ([5, 5, 5], "min", 5, 0),
        ([nan, 5, 1], "max", nan, 0), ([nan, 5, 1], "min", nan, 0),            # a NaN first hit stays
        ([2, nan, 5], "max", 5, 2), ([2, nan, 5], "min", 2, 0),                # a later NaN never wins
        ([-0.0, 0.0], "max", -0.0, 0), ([0.0, -0.0], "min", 0.0, 0),           # -0 == +0: a tie
        ([1, 2, 6], "mean", 3, 2), ([2, nan, 5], "mean", nan, 2)]
    for column, mode, value, k in cases:
        out = run_column(column, mode)
        assert (out["flags"] == HIT).all()
        got = out["value"][0, 0]
        assert np.array_equal(np.float32(got).view(np.uint32), np.float32(value).view(np.uint32)) or \
            (np.isnan(value) and np.isnan(got)), (column, mode, got)
        assert (out["label"] == k).all() and (out["lod"] == 0).all(), (column, mode)
    # the mean is the f32 sum in increasing k, divided by the number of hits
    column = [1e8, 1.0, -1e8, 3.0]
    out = run_column(column, "mean")
    acc = np.float32(0)
    for c in column:
        acc = np.float32(acc + np.float32(c))
    assert out["value"][0, 0] == acc / np.float32(4)


def test_depth_is_the_signed_world_offset_of_the_chosen_sample():
    column = list(range(9))                              # rising with z: max at the top, min at the bottom
    for w, top_depth in (((0.0, 0.0, 1.0), 4.0), ((0.0, 0.0, -1.0), -4.0)):
        for mode, depth in (("max", top_depth), ("min", -top_depth), ("mean", top_depth)):
            out = run_column(column, mode, w)
            assert (out["depth"] == np.float32(depth)).all(), (w, mode, out["depth"])
    # depth scales with |w| (the world length), not with the data-space step: a world that halves z
    mat = material_of({})
    world_inv = np.diag([1.0, 1.0, 2.0, 1.0])             # world z = data z / 2
    out = slab_twin(one_ring(list(range(9))), world_inv, (2, 2, 9), (0.5, 0.5, 2.0), X, Y, (0.0, 0.0, 0.5), 9, "max",
                    2, 2, mat)
    assert (out["depth"] == np.float32(2.0)).all() and (out["value"] == 8).all()
    assert w_len_of((3.0, 4.0, 0.0)) == np.float32(5.0)


def test_axis_slab_plane():
    assert SubVolume.axis_slab_plane("z", (1, 2, 3), 0.5, 2.0) == ((1.0, 2.0, 3.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0),
                                                                  (0.0, 0.0, 2.0))
    assert SubVolume.axis_slab_plane("y", (1, 2, 3)) == ((1.0, 2.0, 3.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
    assert SubVolume.axis_slab_plane(0, (1, 2, 3), 2, 0.25)[1:] == ((0.0, 2.0, 0.0), (0.0, 0.0, 2.0), (0.25, 0.0, 0.0))
    for bad in (dict(axis="w"), dict(step=0), dict(step=-1.0), dict(step=float("inf")), dict(step=1e39),
                dict(pixel_size=0)):
        kw = dict(axis="z", center=(0, 0, 0), pixel_size=1.0, step=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            SubVolume.axis_slab_plane(**kw)


def small_volume():
    d = np.zeros((16, 16, 16), np.uint8)
    return SubVolume(SubVolumeMaterial(0.5), [(d, d)], (2, 2, 2), (4, 4, 4))


def test_render_slab_validation_happens_before_any_device_work(monkeypatch):
    import torch

    vol = small_volume()
    touched = []
    monkeypatch.setattr(vol, "prepare", lambda: touched.append(1))          # the first step that touches the device
    ok = dict(origin=(0, 0, 0), u=(1, 0, 0), v=(0, 1, 0), w=(0, 0, 1), samples=4, width=8, height=6)

    def out_with(**planes):
        base = dict(rgba=torch.empty((6, 8, 4)), depth=None, label=None, flags=None, steps=None)
        base.update(planes)
        return SliceResult(**base)

    cases = [
        (dict(width=0), "width must be an integer >= 1"),
        (dict(origin=(0, float("nan"), 0)), "origin must be three finite numbers"),
        (dict(u=(1, 2, 3), v=(-2, -4, -6)), "u and v must be nonzero and not parallel"),
        (dict(w=(0, 0)), "w must be three finite numbers"),
        (dict(w="abc"), "w must be three finite numbers"),
        (dict(w=(0, 0, float("nan"))), "w must be three finite numbers"),
        (dict(w=(0, 0, 1e39)), "w must be three numbers that are finite in float32"),
        (dict(w=(0, 0, 0)), "w must not be coplanar with u and v"),
        (dict(w=(1, 1, 0)), "w must not be coplanar with u and v"),
        (dict(u=(1e-15, 0, 0), v=(0, 1e-15, 0), w=(0, 0, 1e-20)), "w must not be coplanar with u and v"),   # 0 in float32
        (dict(w=(3e38, 3e38, 3e38)), "w must have a length and a data-space step that are finite in float32"),
        (dict(samples=0), "samples must be an integer in 1 .. 4096"),
        (dict(samples=4097), "samples must be an integer in 1 .. 4096"),
        (dict(samples=2.0), "samples must be an integer in 1 .. 4096"),
        (dict(samples=True), "samples must be an integer in 1 .. 4096"),
        (dict(mode="median"), "mode must be 'max', 'min' or 'mean'"),
        (dict(mode=0), "mode must be 'max', 'min' or 'mean'"),
        (dict(region=FrameRegion.tile(4, 0, 5, 6)), "does not fit"),
        (dict(out=out_with(rgba=torch.empty((6, 8, 3)))), "out.rgba must be a contiguous tensor of shape [6, 8, 4]"),
        (dict(out=out_with()), "out.rgba must be on the volume's GPU device"),
        (dict(out=out_with(lod=torch.empty((8, 6), dtype=torch.uint8))), "out.lod must be a contiguous tensor of shape [6, 8]"),
    ]
    for bad, msg in cases:
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError) as e:
            vol.render_slab(**kw)
        assert msg in str(e.value), (bad, str(e.value))
    # a world transform whose inverse overflows the step in data space
    vol.world.scale = (1e-36, 1.0, 1.0)
    with pytest.raises(ValueError) as e:
        vol.render_slab(**dict(ok, w=(1e3, 0, 1)))
    assert "data-space step" in str(e.value)
    assert not touched


def test_svr_slab_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svr_slab\s*\(", text)
    assert "svr_slab" in _native.SIGNATURES
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "svr_slab")
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", text).group(1)) == 9
    assert ctypes.sizeof(_native.SlabParams) == ctypes.sizeof(_native.SlicePlane) + 4 * 4 + 2 * 4
    for name, value in (("SVR_SLAB_MAX", 0), ("SVR_SLAB_MIN", 1), ("SVR_SLAB_MEAN", 2), ("SVR_SLAB_MAX_SAMPLES", 4096)):
        assert int(re.search(rf"#define {name}\s+(\d+)", text).group(1)) == value
    assert _native.SLAB_MODES == {"max": 0, "min": 1, "mean": 2} and _native.SLAB_MAX_SAMPLES == 4096


def test_infinities_overflow_and_signed_zeros_in_a_column():
    """Hand-written answers for what a float ring may hold: IEEE comparisons and plain f32 sums (include/svr.h)."""
    inf, nan, big = np.float32(np.inf), np.float32(np.nan), np.float32(3e38)
    cases = [  # column, mode, expected value, chosen k (= label)
        ([1, inf, 7, inf], "max", inf, 1), ([1, inf, 7], "min", 1, 0), ([1, -inf, 7, -inf], "min", -inf, 1),
        ([-inf, -5, -inf], "max", -5, 1), ([inf, inf], "min", inf, 0),
        ([1, inf, 7], "mean", inf, 1), ([-inf, 2, 3], "mean", -inf, 2), ([2, inf, -inf, 5], "mean", nan, 1),
        ([0.0, -0.0, 0.0], "max", 0.0, 0), ([-0.0, 0.0, -0.0], "min", -0.0, 0), ([-0.0, -0.0], "mean", 0.0, 0),          # (the sum starts from +0.0)
        ([big, big, 1], "mean", inf, 0), ([big, -big, big], "mean", np.float32(big / np.float32(3)), 0),
        ([big, big, -big, -big], "mean", inf, 0),                                  # inf - 3e38 - 3e38 stays inf
        ([np.float32(1e-41), 0.0], "max", np.float32(1e-41), 0), ([nan, inf], "max", nan, 0), ([inf, nan], "mean", nan, 0)]
    for column, mode, value, k in cases:
        out = run_column(column, mode)
        got = out["value"][0, 0]
        assert (out["flags"] == HIT).all()
        assert np.float32(got).view(np.uint32) == np.float32(value).view(np.uint32) or (np.isnan(value) and np.isnan(got)), \
            (column, mode, got)
        assert (out["label"] == k).all(), (column, mode, out["label"][0, 0])
