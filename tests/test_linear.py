"""Linear sampling without a GPU: the numpy restatement of the linear sample (tests/twin_common.py) against known
answers that do not come from the twin (constants, affine ramps whose trilinear interpolant is the ramp itself, the
nearest slice at voxel centres, the edge texel beyond a window's last voxel centre), a wrapped ring against an
unwrapped one, the material's ``interpolation`` property, the refusal of the march modes under "linear", and
svr_set_interpolation in header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest

from linear_twin import composite_linear, iso_linear, linear_sample, slab_linear, slice_linear, slice_of_spec
from oracle import lmip
from slice_twin import HIT, material_of, slice_twin, twin_of_spec
from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial, _native, testing
from test_slice import moved_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N = 64                                    # a power-of-two volume: ((q + 0.5) / size) * size is exact
EYE = np.eye(4, dtype=f32)
MAT = dict(clim=(0.0, 1.0), gamma=1.0, opacity=1.0, colors=np.array([[0.0, 0.0]], f32))


def ring_of(content, offset, shape, ring, scale=(1.0, 1.0, 1.0)):
    """One LOD's ring dict (the keys of oracle.lmip.rings_of; shader order) holding the window offset / shape of the
    logical array ``content`` [z][y][x] in a ring of ``ring`` slots: slot = logical index mod ring."""
    rx, ry, rz = ring
    density = np.zeros((rz, ry, rx), content.dtype)
    z, y, x = np.meshgrid(*(np.arange(offset[k], offset[k] + shape[k]) for k in (2, 1, 0)), indexing="ij")
    density[z % rz, y % ry, x % rx] = content[z, y, x]
    return dict(density=density, labels=np.zeros((rz, ry, rx), np.uint32), offset=tuple(offset), shape=tuple(shape),
                scale=tuple(scale))


def ramp(dtype, coeff=(3, 5, 7), e=11):
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    return (coeff[0] * x + coeff[1] * y + coeff[2] * z + e).astype(dtype)


def points(lo, hi, step=0.125, seed=0, count=4000):
    """Voxel-index coordinates (centre of voxel i = i) whose fractions are multiples of ``step``, as data points
    d = index + 0.5 in f32."""
    rng = np.random.default_rng(seed)
    idx = [rng.integers(int(lo[k] / step), int(hi[k] / step) + 1, count) * step for k in range(3)]
    return idx, [(i + 0.5).astype(f32) for i in idx]


def test_a_constant_ring_gives_the_constant():
    for dtype, c in ((np.uint8, 200), (np.uint16, 51234), (np.float32, -3.7)):
        ring = ring_of(np.full((N, N, N), c, dtype), (8, 16, 24), (32, 32, 32), (32, 32, 32))
        _, dd = points((8, 16, 24), (39, 47, 55), step=1 / 64)
        value, label, lod = linear_sample([ring], dd)
        assert (lod == 0).all() and (label == 0).all()
        np.testing.assert_array_equal(value, np.full(value.shape, f32(c)))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_an_affine_ramp_is_reproduced_exactly_at_eighths(dtype):
    """Interior points (a voxel away from the window's border) with fractions that are multiples of 1/8: every
    intermediate of the three lerps is a multiple of 1/512 below 2^11, exact in f32, so the value is the ramp's."""
    a, b, c, e = 3, 5, 7, 11
    ring = ring_of(ramp(dtype), (8, 16, 24), (32, 32, 32), (32, 32, 32))       # wrapped on every axis
    idx, dd = points((9, 17, 25), (38, 46, 54))
    value, _, lod = linear_sample([ring], dd)
    assert (lod == 0).all()
    np.testing.assert_array_equal(value, (a * idx[0] + b * idx[1] + c * idx[2] + e).astype(f32))
    assert len(np.unique(np.modf(idx[0])[0])) == 8                             # all eighths occur


def test_the_slice_of_a_ramp_at_pixel_size_one_eighth():
    """The same known answer through the whole slice chain: world == data space, a z-normal plane at z = 30.375."""
    a, b, c, e = 3, 5, 7, 11
    ring = ring_of(ramp(np.uint16), (0, 0, 0), (N, N, N), (N, N, N))
    W = H = 96
    out = slice_linear([ring], EYE, (N, N, N), (20.0625, 33.0625, 30.375), (0.125, 0, 0), (0, 0.125, 0), W, H, MAT,
                       colorspace_srgb=False)
    x = 20.0625 + (np.arange(W) + 0.5 - W / 2) * 0.125
    y = 33.0625 + (np.arange(H) + 0.5 - H / 2) * 0.125
    assert (out["flags"] == HIT).all() and (out["lod"] == 0).all()
    np.testing.assert_array_equal(out["value"], (a * x[None, :] + b * y[:, None] + c * 30.375 + e).astype(f32))


def test_voxel_centres_equal_the_nearest_slice_on_every_plane():
    """Every f is 0 at a voxel centre: bit-identical to slice_twin, over wrapped rings and three LODs."""
    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    for origin, u, v in (((31.5, 31.5, 30.0), (1, 0, 0), (0, 1, 0)), ((31.5, 40.0, 31.5), (1, 0, 0), (0, 0, 1)),
                         ((37.0, 31.5, 31.5), (0, 1, 0), (0, 0, 1))):
        near = twin_of_spec(spec, origin, u, v, N, N, vol=vol)
        lin = slice_of_spec(spec, origin, u, v, N, N, vol=vol)
        assert (near["lod"] == 0).sum() > 200 and (near["lod"] == 1).sum() > 200
        # coarser LODs see these points at fractions of THEIR voxels: compare where LOD 0 answers, everything else alike
        fine = near["lod"] == 0
        for k in ("flags", "label", "lod"):
            np.testing.assert_array_equal(lin[k], near[k])
        np.testing.assert_array_equal(lin["value"][fine].view(np.uint32), near["value"][fine].view(np.uint32))
        np.testing.assert_array_equal(lin["rgba"][fine].view(np.uint32), near["rgba"][fine].view(np.uint32))
    # one LOD: the whole plane
    spec = moved_spec(levels=1)
    vol = lmip.oracle_volume(spec)
    near = twin_of_spec(spec, (31.5, 31.5, 41.0), (1, 0, 0), (0, 1, 0), N, N, vol=vol)
    lin = slice_of_spec(spec, (31.5, 31.5, 41.0), (1, 0, 0), (0, 1, 0), N, N, vol=vol)
    assert (near["flags"] == HIT).sum() > 500
    for k in near:
        np.testing.assert_array_equal(lin[k].view(np.uint8), near[k].view(np.uint8))


def test_beyond_the_last_voxel_centre_the_value_is_the_edge_texel():
    rng = np.random.default_rng(3)
    content = rng.integers(0, 60000, (N, N, N)).astype(np.uint16)
    off, shape = (8, 16, 24), (32, 32, 32)
    ring = ring_of(content, off, shape, (32, 32, 32))
    # x in the last half voxel of the window (and in the first): the cell's two x corners clamp to the edge voxel
    for xv, xedge in ((39.25, 39), (39.4375, 39), (7.625, 8), (7.5, 8)):
        y, z = np.arange(17, 46), 30
        dd = [np.full(y.shape, xv + 0.5, f32), (y + 0.5).astype(f32), np.full(y.shape, z + 0.5, f32)]
        value, _, lod = linear_sample([ring], dd)
        assert (lod == 0).all()
        np.testing.assert_array_equal(value, content[z, y, xedge].astype(f32))
    # a corner of the window: all three axes clamp
    value, _, lod = linear_sample([ring], [np.array([39.4 + 0.5], f32), np.array([47.25 + 0.5], f32), np.array([55.3 + 0.5], f32)])
    assert lod[0] == 0 and value[0] == f32(content[55, 47, 39])
    # the next LOD is not consulted for a corner: with a coarser ring present the fine window still clamps
    coarse = ring_of(np.full((N // 2,) * 3, 7, np.uint16), (0, 0, 0), (32, 32, 32), (32, 32, 32), scale=(0.5, 0.5, 0.5))
    both, _, lod2 = linear_sample([ring, coarse], [np.array([39.4 + 0.5], f32), np.array([47.25 + 0.5], f32), np.array([55.3 + 0.5], f32)])
    assert lod2[0] == 0 and both[0] == value[0]
    outside, _, lod3 = linear_sample([ring, coarse], [np.array([40.25 + 0.5], f32), np.array([30.5], f32), np.array([30.5], f32)])
    assert lod3[0] == 1 and outside[0] == f32(7)


def test_a_wrapped_ring_gives_the_values_of_an_unwrapped_one():
    """The same logical content behind two windows whose ring offsets differ on every axis: identical values wherever
    both hold the cell."""
    rng = np.random.default_rng(5)
    content = rng.normal(100.0, 30.0, (N, N, N)).astype(f32)
    a = ring_of(content, (0, 0, 0), (48, 48, 48), (48, 48, 48))
    b = ring_of(content, (8, 20, 12), (40, 40, 40), (40, 40, 40))
    assert all(o % r for o, r in zip(b["offset"], (40, 40, 40)))
    _, dd = points((9, 21, 13), (46, 46, 46), step=1 / 16, count=6000)
    va, _, la = linear_sample([a], dd)
    vb, _, lb = linear_sample([b], dd)
    assert (la == 0).all() and (lb == 0).all()
    np.testing.assert_array_equal(va.view(np.uint32), vb.view(np.uint32))
    # and through center_on_position: the fly-through's wrapped rings against rings loaded at the last position alone
    moved = moved_spec(levels=1)
    direct = moved_spec(levels=1)
    direct.centers = moved.centers[-1:]
    args = ((40.3, 30.2, 35.1), (0.31, 0.1, 0.0), (0.0, 0.27, 0.12), 80, 60)
    one = slice_of_spec(moved, *args)
    two = slice_of_spec(direct, *args)
    assert (one["flags"] == HIT).sum() > 2000
    for k in one:
        np.testing.assert_array_equal(one[k].view(np.uint8), two[k].view(np.uint8))


def test_the_four_twins_run_with_the_linear_sample():
    import composite_twin
    import iso_twin

    spec = moved_spec()
    vol = lmip.oracle_volume(spec)
    rings = lmip.rings_of(vol)
    size = vol.volume_dimensions_shader
    mat = material_of(spec.material)
    origin, u, v = (30.2, 33.1, 29.7), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7)
    world_inv = spec.world().inverse_matrix
    lin = slice_linear(rings, world_inv, size, origin, u, v, 40, 30, mat)
    near = slice_twin(rings, world_inv, size, origin, u, v, 40, 30, mat)
    slab = slab_linear(rings, world_inv, size, origin, u, v, (0, 0, 1), 1, "max", 40, 30, mat)
    for k in lin:                                           # N = 1, max: the linear slice on every plane
        np.testing.assert_array_equal(slab[k].view(np.uint8), lin[k].view(np.uint8))
    for k in ("flags", "label", "lod"):                     # the LOD pick and the labels are the nearest sample's
        np.testing.assert_array_equal(lin[k], near[k])
    assert (lin["value"] != near["value"]).sum() > 300      # ... the values are not
    M = {k: np.asarray(m, f32) for k, m in spec.matrices().items()}
    table = np.linspace(0, 1, 8, dtype=f32)[:, None].repeat(4, 1)
    comp = composite_linear(rings, M, size, composite_twin.material_of(spec.material), table, 24, 20, 0.95)
    ref = composite_twin.composite_twin(rings, M, size, composite_twin.material_of(spec.material), table, 24, 20, 0.95)
    np.testing.assert_array_equal(comp["flags"] != 0, ref["flags"] != 0)       # the rays are the march's either way
    assert (comp["flags"] == HIT).sum() > 50 and np.abs(comp["rgba"] - ref["rgba"]).max() > 0
    level = 0.45 * float(spec.material.get("clim", (0.0, 1.0))[1])
    iso = iso_linear(rings, M, size, iso_twin.material_of(spec.material), 24, 20, dict(iso_value=level))
    assert (iso["flags"] == HIT).sum() > 50
    n = iso["normal"][iso["flags"] == HIT]
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)


# ---- the Python surface -----------------------------------------------------------------------------------------
def test_material_interpolation_property():
    m = SubVolumeMaterial(0.5)
    assert m.interpolation == "nearest"
    version = m._version
    m.interpolation = "linear"
    assert m.interpolation == "linear" and m._version > version
    m.interpolation = "NEAREST"
    assert m.interpolation == "nearest"
    for bad in ("cubic", "", None, 1):
        with pytest.raises(ValueError, match="interpolation must be one of"):
            m.interpolation = bad
    assert m.interpolation == "nearest"


def small_volume():
    d = np.zeros((16, 16, 16), np.uint8)
    return SubVolume(SubVolumeMaterial(0.5), [(d, d)], (2, 2, 2), (4, 4, 4))


@pytest.mark.parametrize("mode", ["lmip", "mip", "weighted_average"])
def test_the_march_refuses_linear_before_any_device_work(mode, monkeypatch):
    vol = small_volume()
    touched = []
    monkeypatch.setattr(vol, "prepare", lambda: touched.append(1))             # the first step that touches the device
    vol.material.render_mode = mode
    vol.material.interpolation = "linear"
    with pytest.raises(ValueError) as e:
        vol.render(object(), 8, 6)
    msg = str(e.value)
    assert "nearest texels" in msg and "composite" in msg and "iso" in msg and "render_slice" in msg
    assert not touched


def test_render_slice_and_slab_refuse_an_unknown_interpolation(monkeypatch):
    vol = small_volume()
    monkeypatch.setattr(vol, "prepare", lambda: None)
    with pytest.raises(ValueError, match="interpolation must be one of"):
        vol.render_slice((0, 0, 0), (1, 0, 0), (0, 1, 0), 8, 6, interpolation="cubic")
    with pytest.raises(ValueError, match="interpolation must be one of"):
        vol.render_slab((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 3, 8, 6, interpolation="cubic")


def test_svr_set_interpolation_is_declared_bound_and_exported():
    raw = open(os.path.join(ROOT, "include", "svr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+svr_set_interpolation\s*\(\s*svr_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)", text)
    assert re.search(r"#define\s+SVR_INTERP_NEAREST\s+0\b", text) and re.search(r"#define\s+SVR_INTERP_LINEAR\s+1\b", text)
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", text).group(1)) == 9
    assert _native.SIGNATURES["svr_set_interpolation"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _native.INTERPOLATIONS == {"nearest": 0, "linear": 1}
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "svr_set_interpolation")
    # no existing struct gained a field
    assert ctypes.sizeof(_native.SlicePlane) == (16 + 3 * 4) * 4 and ctypes.sizeof(_native.SliceOutputs) == 6 * 8
    assert ctypes.sizeof(_native.CompositeParams) == 8 and ctypes.sizeof(_native.SlabParams) == (16 + 3 * 4) * 4 + 24


def test_non_finite_corners_give_what_the_stated_blend_gives():
    """a + f * (b - a), x first, then y, then z (include/svr.h): a NaN corner at any weight -> NaN; an infinite `b` ->
    that infinity for f > 0 and NaN at f == 0 (0 * inf); an infinite `a` -> NaN at every f.  Only the corner that is the
    `b` of all three steps (v111) can therefore pass an infinity on, and only when every f is above 0."""
    inf, nan, big = np.inf, np.nan, 3e38
    base = (10, 20, 30)                                        # v000 of the cell, (x, y, z)
    cases = [  # {corner offset (dx, dy, dz): value}, fractions (fx, fy, fz), expected
        ({(1, 1, 1): inf}, (0.5, 0.5, 0.5), inf), ({(1, 1, 1): -inf}, (0.25, 0.5, 0.75), -inf),
        ({(1, 1, 1): inf}, (0.0, 0.5, 0.5), nan), ({(1, 1, 1): inf}, (0.5, 0.5, 0.0), nan),      # weight 0 meets an infinity
        ({(1, 1, 1): nan}, (0.0, 0.0, 0.0), nan), ({(0, 1, 0): nan}, (0.5, 0.0, 0.5), nan),      # weight 0 meets a NaN
        ({(0, 0, 0): inf}, (0.5, 0.5, 0.5), nan), ({(0, 0, 0): inf}, (0.0, 0.0, 0.0), nan),      # an infinite `a`
        ({(1, 0, 0): inf}, (0.5, 0.5, 0.5), nan),                                                # `b` in x, then `a` in y
        ({(0, 1, 1): inf, (1, 1, 1): -inf}, (0.5, 0.5, 0.5), nan), ({(0, 1, 1): inf, (1, 1, 1): inf}, (0.5, 0.5, 0.5), nan),
        ({(0, 1, 1): -big, (1, 1, 1): big}, (0.5, 0.5, 0.5), inf),                               # 3e38 - -3e38 overflows
        ({(0, 0, 0): -0.0, (1, 0, 0): -0.0}, (0.5, 0.0, 0.0), 0.0)]            # -0.0 + 0.5 * (+0.0): the zero's sign goes
    for corners, f, want in cases:
        content = np.full((N, N, N), 2.0, f32)
        for (dx, dy, dz), value in corners.items():
            content[base[2] + dz, base[1] + dy, base[0] + dx] = value
        ring = ring_of(content, (0, 0, 0), (N, N, N), (N, N, N))
        value, _, lod = linear_sample([ring], [np.array([base[k] + f[k] + 0.5], f32) for k in range(3)])
        got = f32(value[0])
        assert lod[0] == 0
        assert (np.isnan(want) and np.isnan(got)) or got.view(np.uint32) == f32(want).view(np.uint32), (corners, f, got)
