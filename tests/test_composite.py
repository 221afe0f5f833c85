"""CPU: the composite render mode's restatement (tests/composite_twin.py) against hand-derived answers, the
TransferFunction helpers and their validation, the material switch, and the C declarations (include/svr.h)."""
import math
import os
import re

import numpy as np
import pytest

import ortho_scenes
from composite_twin import composite_twin
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import SubVolumeMaterial, TransferFunction, _native
from sub_volume_renderer_amd._transfer import nominal_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N = 32          # the block's edge in voxels
FRAME = 16      # 16 x 16 pixels at one pixel per voxel: every ray crosses the block along +z


def block_spec():
    d = np.zeros((N, N, N), np.uint8)
    spec = ortho_scenes.base_spec([(d, d.astype(np.uint32))], [(8, 8, 8)], [(4, 4, 4)], width=FRAME, height=FRAME)
    return ortho_scenes.axis_view(spec, "+z")


def ring(density, labels=None, z_range=(0, N)):
    """One LOD whose ring is the whole block (no wrap), with its ROI limited to z in z_range."""
    lab = np.zeros(density.shape, np.uint32) if labels is None else labels
    return dict(density=density.astype(f32), labels=lab, offset=(0, 0, z_range[0]), shape=(N, N, z_range[1] - z_range[0]),
                scale=(1.0, 1.0, 1.0))


def material(**kw):
    m = dict(clim=(0.0, 255.0), opacity=1.0, colors=np.array([(0.0, 0.0), (0.25, 1.0)], f32), clipping_planes=(),
             clipping_mode="ANY")
    m.update(kw)
    return m


def table(rgb, alphas):
    t = np.zeros((len(alphas), 4), f32)
    t[:, :3] = rgb
    t[:, 3] = alphas
    return t


def run(rings, T, cutoff, tint=False, **mat):
    spec = block_spec()
    return composite_twin(rings, spec.matrices(), (f32(N),) * 3, material(**mat), T, FRAME, FRAME, cutoff, tint)


def nsteps_and_dz(spec):
    """float64 number of samples and the z voxel coordinate of every sample of the rays (which cross z = -0.5 ..
    N - 0.5 with x, y fixed): the march's nsteps = trunc(N / rel_step + 0.5), samples evenly spaced from the entry."""
    rel = float(nominal_step((N, N, N)))
    n = int(N / rel + 0.5)
    return n, np.arange(n) * (N / n)


def test_uniform_block_accumulates_one_minus_transmittance():
    a = 0.05
    T = table((0.2, 0.6, 0.9), [a, a, a])
    dens = np.full((N, N, N), 100.0)
    n, _ = nsteps_and_dz(block_spec())
    # cutoff 0.99: the first n with 1 - (1 - a)^n >= 0.99 (90; the block gives about 113 samples)
    expect_n = math.ceil(math.log(0.01) / math.log(1.0 - a))
    assert 1.0 - (1.0 - a) ** (expect_n - 1) < 0.99 - 1e-4 and expect_n < n
    out = run([ring(dens)], T, 0.99)
    assert (out["flags"] == HIT).all()
    assert (out["steps"] == expect_n).all()
    np.testing.assert_allclose(out["rgba"][..., 3], 1.0 - (1.0 - a) ** expect_n, atol=2e-6)
    np.testing.assert_allclose(out["rgba"][..., :3], np.broadcast_to(f32((0.2, 0.6, 0.9)), (FRAME, FRAME, 3)), atol=2e-6)
    # cutoff 1.0 visits every sample
    out = run([ring(dens)], T, 1.0)
    assert (out["steps"] == n).all()
    np.testing.assert_allclose(out["rgba"][..., 3], 1.0 - (1.0 - a) ** n, atol=2e-6)
    # best: the largest w is the first sample's (w falls with the transmittance); its pick holds the entry coordinate
    assert (out["pick"] >> np.uint64(48) == 0).all()


def test_opaque_first_sample_gives_its_colour_depth_and_one_step():
    spec = block_spec()
    T = table((0.9, 0.3, 0.1), [1.0, 1.0])
    out = run([ring(np.full((N, N, N), 7.0))], T, 0.99, opacity=0.5)
    assert (out["flags"] == HIT).all() and (out["steps"] == 1).all()
    np.testing.assert_allclose(out["rgba"], np.broadcast_to(f32((0.9, 0.3, 0.1, 0.5)), (FRAME, FRAME, 4)), atol=1e-7)
    # depth of the first sample, the entry point z = -0.5 (normalised coordinate c = (d + 0.5) / N, so c_z = 0), by the
    # march's formula: the world image of c - 0.5, projected; in float64
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    near, _ = ortho_scenes.pixel_rays(spec)
    c = [(near[0] + 0.5) / N, (near[1] + 0.5) / N, np.zeros_like(near[0])]
    p = np.stack([c[0] - 0.5, c[1] - 0.5, c[2] - 0.5, np.ones_like(near[0])])
    clip = np.einsum("rc,chw->rhw", M["proj"] @ M["cam"] @ M["world"], p)
    np.testing.assert_allclose(out["depth"], clip[2] / clip[3], atol=1e-5)


def test_samples_no_lod_holds_are_skipped():
    spec = block_spec()
    n, dz = nsteps_and_dz(spec)
    assert np.abs(dz - 8.0).min() > 1e-3 and np.abs(dz - 24.0).min() > 1e-3
    # opaque table, ROI from z = 8: the first resident sample ends the ray
    first = int(np.argmax(dz >= 8.0))
    T = table((1.0, 1.0, 1.0), [1.0, 1.0])
    out = run([ring(np.full((N, N, N), 3.0), z_range=(8, N))], T, 0.99)
    assert (out["flags"] == HIT).all() and (out["steps"] == first + 1).all()
    # a faint table over ROI z in [8, 24): only the resident samples add opacity, every sample is counted
    a = 0.03
    out = run([ring(np.full((N, N, N), 3.0), z_range=(8, 24))], table((1, 1, 1), [a, a]), 1.0)
    resident = int(((dz >= 8.0) & (dz < 24.0)).sum())
    assert (out["steps"] == n).all()
    np.testing.assert_allclose(out["rgba"][..., 3], 1.0 - (1.0 - a) ** resident, atol=2e-6)
    # nothing resident along the ray: a transparent miss
    out = run([ring(np.full((N, N, N), 3.0), z_range=(0, 0))], T, 0.99)
    assert (out["flags"] == MISS).all() and (out["steps"] == n).all()
    assert not out["rgba"].any() and not out["depth"].any() and not out["label"].any() and not out["pick"].any()


def test_nan_maps_to_entry_zero_and_values_clamp():
    T = table((0.0, 0.0, 0.0), [0.0, 0.0, 0.0])
    T[0] = (0.8, 0.1, 0.2, 0.5)
    out = run([ring(np.full((N, N, N), np.nan))], T, 0.99)
    assert (out["flags"] == HIT).all() and (out["steps"] == 7).all()          # 1 - 0.5^7 >= 0.99 > 1 - 0.5^6
    np.testing.assert_allclose(out["rgba"][..., :3], np.broadcast_to(f32((0.8, 0.1, 0.2)), (FRAME, FRAME, 3)), atol=1e-6)
    # below clim[0]: entry 0; above clim[1]: entry K-1
    T[-1] = (0.0, 0.0, 1.0, 1.0)
    assert (run([ring(np.full((N, N, N), -40.0))], T, 0.99)["steps"] == 7).all()
    out = run([ring(np.full((N, N, N), 1e6))], T, 0.99)
    assert (out["steps"] == 1).all() and np.array_equal(out["rgba"][0, 0], f32((0.0, 0.0, 1.0, 1.0)))
    # halfway between entries 0 and 1 of a K = 3 table: the mean of the two
    T = table((0.0, 0.0, 0.0), [0.0, 1.0, 1.0])
    out = run([ring(np.full((N, N, N), 63.75))], T, 0.99)                      # v = 0.25 -> x = 0.5
    assert (out["steps"] == 7).all()


def test_label_tint():
    labels = np.ones((N, N, N), np.uint32)
    T = table((1.0, 1.0, 1.0), [0.2, 0.2])
    plain = run([ring(np.full((N, N, N), 50.0), labels)], T, 0.99)
    tinted = run([ring(np.full((N, N, N), 50.0), labels)], T, 0.99, tint=True)
    # colors[1] = (h 0.25, s 1): hsv_to_rgb(0.25, 1, 1) = (0.5, 1, 0)
    np.testing.assert_allclose(tinted["rgba"][..., :3], np.broadcast_to(f32((0.5, 1.0, 0.0)), (FRAME, FRAME, 3)), atol=1e-6)
    np.testing.assert_allclose(plain["rgba"][..., :3], 1.0, atol=1e-6)
    for k in ("steps", "label", "depth", "flags"):
        assert np.array_equal(plain[k], tinted[k]), k
    assert (plain["label"] == 1).all()
    # label 2 wraps onto colors[0] (grey: s = 0)
    tinted = run([ring(np.full((N, N, N), 50.0), labels * 2)], T, 0.99, tint=True)
    np.testing.assert_allclose(tinted["rgba"][..., :3], 1.0, atol=1e-6)


def test_clipping_planes_discard_like_the_march():
    T = table((1, 1, 1), [0.1, 0.1])
    dens = np.full((N, N, N), 3.0)
    spec = block_spec()
    cx = float(np.asarray(spec.cam_position)[0])
    out = run([ring(dens)], T, 0.99, clipping_planes=[(1.0, 0.0, 0.0, cx)])
    assert (out["flags"] == DISCARD).any() and (out["flags"] == HIT).any()
    assert not out["rgba"][out["flags"] == DISCARD].any()
    both = run([ring(dens)], T, 0.99, clipping_planes=[(1.0, 0.0, 0.0, cx), (-1.0, 0.0, 0.0, -cx)], clipping_mode="ALL")
    assert not (both["flags"] == DISCARD).any()


# ---- TransferFunction ----------------------------------------------------------------------------------------
def test_transfer_function_construction_and_helpers():
    t = np.linspace(0, 1, 40).reshape(10, 4)
    tf = TransferFunction(t)
    assert tf.size == 10 and tf.table.dtype == np.float64 and np.array_equal(tf.table, t)
    with pytest.raises(ValueError):
        tf.table[0, 0] = 1.0                                     # read-only
    s = TransferFunction(t, srgb=True)
    c = t[:, :3]
    np.testing.assert_allclose(s.table[:, :3], np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4))
    assert np.array_equal(s.table[:, 3], t[:, 3])

    lin = TransferFunction.linear()
    assert lin.size == 256 and np.array_equal(lin.table[:, :3], np.ones((256, 3)))
    np.testing.assert_allclose(lin.table[:, 3], 0.05 * np.arange(256) / 255.0)
    lin = TransferFunction.linear(color=(0.1, 0.2, 0.3), opacity=0.5, size=2)
    assert np.array_equal(lin.table, [[0.1, 0.2, 0.3, 0.0], [0.1, 0.2, 0.3, 0.5]])

    pts = TransferFunction.from_points([(0.25, (1, 0, 0, 0)), (0.75, (0, 0, 1, 1))], size=5)
    np.testing.assert_allclose(pts.table, [[1, 0, 0, 0], [1, 0, 0, 0], [0.5, 0, 0.5, 0.5], [0, 0, 1, 1], [0, 0, 1, 1]])
    one = TransferFunction.from_points([(0.3, (0.2, 0.4, 0.6, 0.8))], size=3)
    assert np.array_equal(one.table, np.tile([0.2, 0.4, 0.6, 0.8], (3, 1)))


def test_device_table_corrects_alpha_for_the_nominal_step():
    t = np.array([[0.1, 0.2, 0.3, 0.0], [0.4, 0.5, 0.6, 0.3], [0.7, 0.8, 0.9, 1.0]])
    tf = TransferFunction(t)
    for dims, rel in (((64, 64, 64), 0.4), ((10, 20, 30), 0.273861), ((1, 1, 2), 0.1), ((4096, 8, 8), 0.8)):
        assert nominal_step(dims) == f32(min(max(np.sqrt(f32(max(dims))) / f32(20), f32(0.1)), f32(0.8)))
        assert abs(float(nominal_step(dims)) - rel) < 1e-6
        d = tf.device_table(dims)
        assert d.dtype == np.float32 and d.shape == (3, 4) and d.flags.c_contiguous
        assert np.array_equal(d[:, :3], t[:, :3].astype(f32))
        r = float(nominal_step(dims))
        assert np.array_equal(d[:, 3], (1.0 - (1.0 - t[:, 3]) ** r).astype(f32))
        assert d[0, 3] == 0.0 and d[2, 3] == 1.0
    # one voxel of material composited over 1 / rel_step samples gives the table's alpha
    d = tf.device_table((64, 64, 64))
    assert abs((1.0 - (1.0 - float(d[1, 3])) ** (1 / 0.4)) - 0.3) < 1e-6


@pytest.mark.parametrize("bad", [
    np.zeros((1, 4)), np.zeros((4097, 4)), np.zeros((4, 3)), np.zeros(8), [[0, 0, 0, 1.5], [0, 0, 0, 0]],
    [[0, 0, 0, -0.1], [0, 0, 0, 0]], [[0, 0, np.nan, 0], [0, 0, 0, 0]], [[0, 0, np.inf, 0], [0, 0, 0, 0]], "table",
    [[0, 0, 0, "a"], [0, 0, 0, 0]],
])
def test_transfer_function_refuses_bad_tables(bad):
    with pytest.raises(ValueError):
        TransferFunction(bad)


def test_transfer_function_helpers_refuse_bad_arguments():
    for kw in (dict(size=1), dict(size=4097), dict(size=2.5), dict(size=True), dict(color=(1, 1)), dict(color="red"),
               dict(opacity=1.5), dict(opacity="x"), dict(opacity=-0.1)):
        with pytest.raises(ValueError):
            TransferFunction.linear(**kw)
    for points in ([], "ab", [(0.5,)], [(1.5, (0, 0, 0, 0))], [(0.5, (0, 0, 0))], [(0.6, (0, 0, 0, 0)), (0.4, (0, 0, 0, 0))],
                   [(0.5, (0, 0, 0, 2))], [(float("nan"), (0, 0, 0, 0))], [(0.5, "rgba")]):
        with pytest.raises(ValueError):
            TransferFunction.from_points(points)
    with pytest.raises(ValueError):
        TransferFunction.from_points([(0.0, (0, 0, 0, 0))], size=0)


# ---- the material switch --------------------------------------------------------------------------------------
def test_material_composite_mode_and_its_properties():
    m = SubVolumeMaterial(lmip_threshold=0.5)
    assert "composite" in SubVolumeMaterial.RENDER_MODES
    assert m.transfer_function is None and m.alpha_cutoff == pytest.approx(0.99) and m.color_by_label is False
    assert m.effective_transfer_function() is m.effective_transfer_function()
    assert np.array_equal(m.effective_transfer_function().table, TransferFunction.linear().table)
    v = m._version
    m.render_mode = "COMPOSITE"
    assert m.render_mode == "composite" and m._version > v
    tf = TransferFunction.linear(opacity=0.2)
    for name, value in (("transfer_function", tf), ("alpha_cutoff", 1.0), ("alpha_cutoff", 0.5), ("color_by_label", True),
                        ("transfer_function", None)):
        v = m._version
        setattr(m, name, value)
        assert getattr(m, name) == value and m._version > v, name
    m.transfer_function = tf
    assert m.effective_transfer_function() is tf
    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf"), "0.5", None, 1e-50):
        with pytest.raises(ValueError):
            m.alpha_cutoff = bad
    for bad in (np.zeros((4, 4)), "linear", 3):
        with pytest.raises(ValueError):
            m.transfer_function = bad
    with pytest.raises(ValueError):
        m.render_mode = "fading"
    # the LMIP uniforms are sent unchanged in composite mode (svr_composite does not read them)
    assert m.lmip_uniforms() == (0.5, 0.5, 10)


# ---- the C declarations ---------------------------------------------------------------------------------------
def test_header_declares_the_composite_entry_points_within_abi_9():
    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert re.search(r"#define SVR_ABI_VERSION 9\b", header)
    assert re.search(r"int\s+svr_set_transfer_function\(svr_ctx\* ctx, const float\* rgba, int32_t K\);", header)
    assert re.search(r"int\s+svr_composite\(svr_ctx\* ctx, const svr_camera\* cam, const svr_frame\* frame, "
                     r"const svr_composite_params\* params,\s+const svr_outputs\* out, void\* stream\);", header)
    body = re.search(r"typedef struct svr_composite_params \{(.*?)\} svr_composite_params;", header, re.S).group(1)
    assert re.findall(r"(float|int32_t)\s+(\w+);", body) == [("float", "alpha_cutoff"), ("int32_t", "color_by_label")]
    assert re.search(r"#define SVR_TF_MAX_ENTRIES 4096\b", header) and _native.TF_MAX_ENTRIES == 4096
    assert {"svr_set_transfer_function", "svr_composite"} <= set(_native.SIGNATURES)
    assert [n for n, _ in _native.CompositeParams._fields_] == ["alpha_cutoff", "color_by_label"]


def test_table_entries_of_infinite_negative_and_out_of_range_samples():
    """x = fminf(fmaxf(v * (K-1), 0), K-1): NaN and everything below clim[0] (-inf included) take entry 0, +inf and
    everything above clim[1] entry K-1; the order of the two clamps matters only for NaN (fminf first would give K-1)."""
    T = table((0.0, 0.0, 0.0), [0.0, 0.0, 0.0])
    T[0], T[-1] = (0.8, 0.1, 0.2, 0.5), (0.0, 0.0, 1.0, 1.0)
    first, last = f32((0.8, 0.1, 0.2)), f32((0.0, 0.0, 1.0))
    for value, steps, rgb in ((np.nan, 7, first), (-np.inf, 7, first), (-3e38, 7, first), (-0.0, 7, first),
                              (np.inf, 1, last), (3e38, 1, last), (1e6, 1, last)):
        out = run([ring(np.full((N, N, N), value, np.float32))], T, 0.99)
        assert (out["flags"] == HIT).all() and (out["steps"] == steps).all(), (value, out["steps"][0, 0])
        np.testing.assert_allclose(out["rgba"][..., :3], np.broadcast_to(rgb, (FRAME, FRAME, 3)), atol=1e-6, err_msg=str(value))
        assert np.isfinite(out["rgba"]).all() and np.isfinite(out["depth"]).all()
        assert out["saw_nan"].all() == bool(np.isnan(value)) and out["saw_pinf"].all() == (value == np.inf)
