"""Cross-section views without a GPU: the numpy restatement of svr_slice (tests/slice_twin.py) against known answers
read from the SOURCE arrays (not from the rings it samples), every host-side refusal of SubVolume.render_slice, the
axis-aligned plane helper, and the C entry point in header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest

import sub_volume_renderer_amd as svr
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, twin_of_spec
from sub_volume_renderer_amd import FrameRegion, SliceResult, SubVolume, SubVolumeMaterial, _native, testing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


def moved_spec(levels=3):
    """64^3 synthetic scene after a fly-through of center_on_position calls that leaves the rings wrapped."""
    spec = testing.synthetic_spec(N)
    if levels < 3:
        spec.pairs, spec.chunk_shapes, spec.ring_shapes = spec.pairs[:levels], spec.chunk_shapes[:levels], spec.ring_shapes[:levels]
    spec.centers = [((20.0, 24.0, 30.0), None), ((37.0, 33.0, 41.0), None), ((44.5, 29.0, 35.0), None)]
    return spec


def expected_from_sources(spec, vol, d):
    """Value / LOD of the data-space voxels d (int arrays, shader order) read from the source arrays: the first
    level whose ROI holds floor(d * scale)."""
    value = np.zeros(d[0].shape, np.float32)
    lod = np.full(d[0].shape, 255, np.uint8)
    done = np.zeros(d[0].shape, bool)
    for l, ((data, _), b) in enumerate(zip(spec.pairs, vol.wrapping_buffers)):
        u = b.uniform()
        ic = [np.floor(d[k] * np.float32(u["scale"][k])).astype(np.int64) for k in range(3)]
        inb = ~done
        for k in range(3):
            inb &= (u["offset"][k] <= ic[k]) & (ic[k] < u["offset"][k] + u["shape"][k])
        value[inb] = data[ic[2][inb], ic[1][inb], ic[0][inb]]
        lod[inb] = l
        done |= inb
    return value, lod


def test_z_normal_slice_on_voxel_centres_shows_the_source_voxels_after_wrapping_moves():
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    wraps = [int(o) % r for b in vol.wrapping_buffers for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1])]
    assert any(wraps), "the moves must leave nonzero ring wrap offsets"
    for z in (3, 30, 41, 62):
        # 64 x 64 pixels of size 1: pixel (x, y) centre = (x, y, z) exactly when origin = (31.5, 31.5, z)
        out = twin_of_spec(spec, (31.5, 31.5, float(z)), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), N, N, vol=vol)
        yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        value, lod = expected_from_sources(spec, vol, (xx, yy, np.full_like(xx, z)))
        np.testing.assert_array_equal(out["value"], value)
        np.testing.assert_array_equal(out["lod"], lod)
        np.testing.assert_array_equal(out["flags"], np.where(lod == 255, MISS, HIT))
        labels = spec.pairs[0][1]
        np.testing.assert_array_equal(out["label"][lod == 0], labels[z, yy[lod == 0], xx[lod == 0]])
        assert not out["depth"].any()
    # the scene has LOD 0 and LOD 1 voxels on the planes through the window
    out = twin_of_spec(spec, (31.5, 31.5, 41.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), N, N, vol=vol)
    assert (out["lod"] == 0).sum() > 200 and (out["lod"] == 1).sum() > 200


def test_outside_the_box_is_discard_and_inside_but_not_resident_is_miss():
    spec = moved_spec(levels=1)                             # one level whose window is smaller than the volume
    vol = lmip.oracle_volume(spec)
    out = twin_of_spec(spec, (31.5, 31.5, 40.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 96, 96, vol=vol)
    x = np.arange(96) - 16                                  # data-space x of each column (and y of each row)
    outside = (x[None, :] < 0) | (x[None, :] >= N) | (x[:, None] < 0) | (x[:, None] >= N)
    np.testing.assert_array_equal(out["flags"] == DISCARD, outside)
    assert not out["rgba"][outside].any() and (out["lod"][outside] == 255).all()
    miss = out["flags"] == MISS
    assert miss.sum() > 500 and (out["flags"] == HIT).sum() > 500
    assert (out["lod"][miss] == 255).all() and not out["value"][miss].any() and not out["label"][miss].any()
    np.testing.assert_array_equal(out["rgba"][miss], np.tile([0, 0, 0, 1], (int(miss.sum()), 1)))
    hit = out["flags"] == HIT
    assert (out["rgba"][hit][:, 3] == 1.0).all()           # opacity of the default material
    # a plane wholly outside the box
    out = twin_of_spec(spec, (31.5, 31.5, -3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 8, 8, vol=vol)
    assert (out["flags"] == DISCARD).all()


def test_pixel_centres_on_the_faces_of_the_box():
    """-0.5 is inside (c = 0), size - 0.5 is outside (c = 1): 0 <= dx < size."""
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    low = twin_of_spec(spec, (31.5, 31.5, -0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), N, N, vol=vol)
    assert (low["flags"] != DISCARD).all()
    high = twin_of_spec(spec, (31.5, 31.5, N - 0.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), N, N, vol=vol)
    assert (high["flags"] == DISCARD).all()
    # columns: pixel centres at x = -0.5, 0.5, ..., 64.5 (origin 31.5 - 0.5 with an odd width of 67 pixels -> first at -1.5)
    out = twin_of_spec(spec, (31.5, 31.5, 30.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 67, N, vol=vol)
    xs = np.arange(67) - 33 + 31.5                         # -1.5 .. 64.5
    inside_cols = (xs >= -0.5) & (xs < N - 0.5)
    np.testing.assert_array_equal((out["flags"] != DISCARD).all(axis=0), inside_cols)
    np.testing.assert_array_equal((out["flags"] == DISCARD).all(axis=0), ~inside_cols)


def test_regions_of_the_twin_assemble_to_the_full_frame():
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    args = ((30.2, 33.1, 29.7), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7), 50, 38)
    full = twin_of_spec(spec, *args, vol=vol)
    r = FrameRegion.stripes(50, 38, 1, 3, band_h=4)
    part = twin_of_spec(spec, *args, vol=vol, region=r)
    rows = [y for y in range(38) if (y // 4) % 3 == 1]
    np.testing.assert_array_equal(part["value"][:len(rows)], full["value"][rows])
    assert (part["flags"][len(rows):] == DISCARD).all()      # padding rows


def test_axis_slice_plane():
    assert SubVolume.axis_slice_plane("z", (1, 2, 3), 0.5) == ((1.0, 2.0, 3.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0))
    assert SubVolume.axis_slice_plane("y", (1, 2, 3), 2) == ((1.0, 2.0, 3.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0))
    assert SubVolume.axis_slice_plane(0, (1, 2, 3)) == ((1.0, 2.0, 3.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    for bad in (dict(axis="w"), dict(axis=3), dict(axis=True), dict(pixel_size=0), dict(pixel_size=float("nan")),
                dict(center=(0, 0))):
        kw = dict(axis="z", center=(0, 0, 0), pixel_size=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            SubVolume.axis_slice_plane(**kw)


def small_volume():
    d = np.zeros((16, 16, 16), np.uint8)
    return SubVolume(SubVolumeMaterial(0.5), [(d, d)], (2, 2, 2), (4, 4, 4))


def test_render_slice_validation_happens_before_any_device_work(monkeypatch):
    import torch

    vol = small_volume()
    touched = []
    monkeypatch.setattr(vol, "prepare", lambda: touched.append(1))          # the first step that touches the device
    ok = dict(origin=(0, 0, 0), u=(1, 0, 0), v=(0, 1, 0), width=8, height=6)

    def out_with(**planes):
        base = dict(rgba=torch.empty((6, 8, 4)), depth=None, label=None, flags=None, steps=None)
        base.update(planes)
        return SliceResult(**base)

    cases = [
        (dict(width=0), "width must be an integer >= 1"),
        (dict(height=-2), "height must be an integer >= 1"),
        (dict(width=2.5), "width must be an integer >= 1"),
        (dict(origin=(0, 0)), "origin must be three finite numbers"),
        (dict(origin=(0, float("nan"), 0)), "origin must be three finite numbers"),
        (dict(u=(1, 0, float("inf"))), "u must be three finite numbers"),
        (dict(v="abc"), "v must be three finite numbers"),
        (dict(u=(0, 0, 0)), "u and v must be nonzero and not parallel"),
        (dict(v=(0, 0, 0)), "u and v must be nonzero and not parallel"),
        (dict(u=(1, 2, 3), v=(-2, -4, -6)), "u and v must be nonzero and not parallel"),
        (dict(region=FrameRegion.tile(4, 0, 5, 6)), "does not fit"),
        (dict(region=FrameRegion.tile(0, 2, 8, 5)), "does not fit"),
        (dict(region=FrameRegion.tile(-1, 0, 4, 4)), "does not fit"),
        (dict(region=FrameRegion(0, 6, 8, 4, 2, 4)), "does not fit"),
        (dict(out=out_with(rgba=torch.empty((6, 8, 3)))), "out.rgba must be a contiguous tensor of shape [6, 8, 4]"),
        (dict(out=out_with(rgba=torch.empty((6, 8, 4), dtype=torch.float64))), "out.rgba must have dtype float32"),
        (dict(out=out_with()), "out.rgba must be on the volume's GPU device"),
        (dict(out=out_with(rgba=None)), "out.rgba is required"),
        (dict(out=out_with(value=torch.empty((6, 8), dtype=torch.int32))), "out.value must have dtype float32"),
        (dict(out=out_with(lod=torch.empty((8, 6), dtype=torch.uint8))), "out.lod must be a contiguous tensor of shape [6, 8]"),
        (dict(out=out_with(label=torch.empty((6, 8), dtype=torch.int32))), "out.rgba must be on the volume's GPU device"),
        (dict(region=FrameRegion.tile(0, 0, 4, 3), out=out_with()), "out.rgba must be a contiguous tensor of shape [3, 4, 4]"),
        (dict(out=svr.RenderResult(torch.empty((6, 8, 4)), None, None, None, None)), "out must be a SliceResult"),
    ]
    for bad, msg in cases:
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError) as e:
            vol.render_slice(**kw)
        assert msg in str(e.value), (bad, str(e.value))
    assert not touched


def test_slice_result_is_a_render_result():
    assert issubclass(SliceResult, svr.RenderResult) and "SliceResult" in svr.__all__
    r = SliceResult(rgba=1, depth=2, label=3, flags=4, steps=None)
    assert r.pick is None and r.value is None and r.lod is None


def test_svr_slice_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+svr_slice\s*\(", text)
    assert "svr_slice" in _native.SIGNATURES
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "svr_slice")
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", text).group(1)) == 9
    assert ctypes.sizeof(_native.SlicePlane) == (16 + 3 * 4) * 4 and ctypes.sizeof(_native.SliceOutputs) == 6 * 8


def test_a_slice_passes_every_float_through_bit_for_bit():
    """value is the texel itself (include/svr.h): NaN with its payload, +-inf, -0.0, a subnormal and +-3e38 arrive as
    their bits; the rgba of each follows from the stated shading chain."""
    from slice_twin import material_of, slice_twin

    bits = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00001BE0, 0x7F61B1E6, 0xFF61B1E6], np.uint32)
    d = np.resize(bits, (8, 8, 8)).view(np.float32).copy()
    ring = dict(density=d, labels=np.zeros((8, 8, 8), np.uint32), offset=(0, 0, 0), shape=(8, 8, 8), scale=(1.0, 1.0, 1.0))
    out = slice_twin([ring], np.eye(4), (8, 8, 8), (3.5, 3.5, 2.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 8, 8, material_of({}))
    assert (out["flags"] == HIT).all()
    np.testing.assert_array_equal(out["value"].view(np.uint32), d[2].view(np.uint32))
    v = out["value"]
    assert np.isnan(out["rgba"][np.isnan(v)][:, :3]).all() and (out["rgba"][..., 3] == 1.0).all()
    assert np.isinf(out["rgba"][v == np.inf][:, :3]).any(-1).all()
