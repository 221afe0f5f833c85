"""CPU: the iso-surface mode's restatement (tests/iso_twin.py) against hand-derived answers that need no tolerance
argument, the material's iso properties and their validation, and the C declarations (include/svr.h)."""
import math
import os
import re

import numpy as np
import pytest

import ortho_scenes
from iso_twin import iso_twin
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import IsoResult, RenderResult, SubVolumeMaterial, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N = 32          # the block's edge in voxels
FRAME = 16      # 16 x 16 pixels at one pixel per voxel
NSTEPS = 113    # trunc(32 / rel_step + 0.5), rel_step = sqrt(32) / 20: sample i sits at data coordinate i * 32 / 113
SHADE = dict(ambient=0.25, diffuse=0.5, specular=0.125, shininess_log2=2, iso_color=(0.5, 1.0, 0.25), refine=0)


def spec_for(view="+x", world_scale=(1.0, 1.0, 1.0)):
    d = np.zeros((N, N, N), np.uint8)
    spec = ortho_scenes.base_spec([(d, d.astype(np.uint32))], [(8, 8, 8)], [(4, 4, 4)], width=FRAME, height=FRAME)
    spec.world_scale = world_scale
    return ortho_scenes.axis_view(spec, view) if isinstance(view, str) else view(spec)


def ring(density, labels=None, z_range=None, scale=1.0):
    """One LOD whose ring is its whole array (no wrap), with its ROI limited to z in z_range."""
    n = density.shape[0]
    z_range = z_range or (0, n)
    lab = np.zeros(density.shape, np.uint32) if labels is None else labels
    return dict(density=density.astype(f32), labels=lab, offset=(0, 0, z_range[0]), shape=(n, n, z_range[1] - z_range[0]),
                scale=(scale,) * 3)


def material(**kw):
    m = dict(opacity=0.75, colors=np.array([(0.0, 0.0), (0.25, 1.0)], f32), clipping_planes=(), clipping_mode="ANY")
    m.update(kw)
    return m


def run(rings, spec, **params):
    p = dict(SHADE)
    p.update(params)
    return iso_twin(rings, spec.matrices(), (f32(N),) * 3, material(), FRAME, FRAME, p, pick_id=5)


def step_along_x(first_dense=10, below=False):
    """[z, y, x] block: 200 for x >= first_dense (or, with below, for x < first_dense), else 0."""
    d = np.zeros((N, N, N), np.uint8)
    if below:
        d[:, :, :first_dense] = 200
    else:
        d[:, :, first_dense:] = 200
    return d


def angled(spec):
    """An orthographic camera whose rays travel along (0.6, 0.8, 0) through the block's centre."""
    spec.projection, spec.ortho_size, spec.depth_range = "orthographic", (12.0, 12.0), (1.0, 200.0)
    c = np.array([15.5, 15.5, 15.5])
    spec.cam_position, spec.cam_target = tuple(c - 60.0 * np.array([0.6, 0.8, 0.0])), tuple(c)
    return spec


def depth_by_hand(spec, coord):
    """The march's depth formula in float64: NDC z of world * (coord - 0.5) (normalised coordinate, as the shader has it)."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    p = M["proj"] @ M["cam"] @ M["world"] @ np.array([coord[0] - 0.5, coord[1] - 0.5, coord[2] - 0.5, 1.0])
    return p[2] / max(p[3], 0.001)


def test_a_step_seen_head_on_hits_at_the_plane_with_the_axis_normal():
    spec = spec_for("+x")
    out = run([ring(step_along_x(10))], spec, iso_value=100.0)
    assert (out["flags"] == HIT).all()
    # sample 35 sits at x = 9.91 (voxel 9), sample 36 at 10.19 (voxel 10): the first at the level is 36
    assert (out["steps"] == 37).all() and (out["iter"] == 36.0).all()
    assert np.array_equal(out["normal"], np.broadcast_to(np.array([-1.0, 0.0, 0.0], f32), (FRAME, FRAME, 3)))
    # n = v = l = h: |n.l| = |n.h| = 1, so rgb = base * (ambient + diffuse) + specular exactly
    assert np.array_equal(out["rgba"], np.broadcast_to(np.array([0.5 * 0.75 + 0.125, 0.75 + 0.125, 0.25 * 0.75 + 0.125, 0.75], f32),
                                                       (FRAME, FRAME, 4)))
    x = 36.0 * (1.0 / NSTEPS)                                # normalised x of the hit; y, z of pixel (0, 0) from its pick word
    word = int(out["pick"][0, 0])
    assert word & 0xFFFFF == 5 and (word >> 20) & 0x3FFF == int(x * 16383.0)
    for (j, i) in ((0, 0), (7, 9), (15, 15)):
        cy, cz = (15.5 + 0.5 + (i + 0.5 - 8.0)) / N, (15.5 + 0.5 - (j + 0.5 - 8.0)) / N
        assert abs(float(out["depth"][j, i]) - depth_by_hand(spec, (x, cy, cz))) < 1e-6
    assert (out["label"] == 0).all()
    # from the other side the dense half faces -x... seen along -x the surface of "dense below x = 22" faces +x
    out = run([ring(step_along_x(22, below=True))], spec_for("-x"), iso_value=100.0)
    assert (out["flags"] == HIT).all()
    assert np.array_equal(out["normal"], np.broadcast_to(np.array([1.0, 0.0, 0.0], f32), (FRAME, FRAME, 3)))


def test_a_step_seen_at_a_known_angle_shades_with_the_cosine():
    spec = spec_for(angled)
    out = run([ring(step_along_x(10))], spec, iso_value=100.0)
    on_plane = (out["normal"] == np.array([-1.0, 0.0, 0.0], f32)).all(-1)
    assert on_plane.sum() > 60                               # rays that enter through the empty half and meet the plane
    # v = l = h = (-0.6, -0.8, 0): |n.l| = |n.h| = 0.6, specular power 2^2
    t, s = 0.25 + 0.5 * 0.6, 0.125 * 0.6 ** 4
    want = np.array([0.5 * t + s, 1.0 * t + s, 0.25 * t + s, 0.75])
    assert np.abs(out["rgba"][on_plane] - want).max() < 2e-6
    # a fixed light instead of the headlight: l = (-1, 0, 0) gives |n.l| = 1; h = normalize(l + v) = (-1.6, -0.8, 0) / sqrt(3.2)
    out = run([ring(step_along_x(10))], spec, iso_value=100.0, light_direction=(-1.0, 0.0, 0.0))
    t, s = 0.25 + 0.5, 0.125 * (1.6 / math.sqrt(3.2)) ** 4
    assert np.abs(out["rgba"][on_plane] - np.array([0.5 * t + s, t + s, 0.25 * t + s, 0.75])).max() < 2e-6


def test_a_volume_below_the_level_misses_everywhere():
    out = run([ring(np.full((N, N, N), 99, np.uint8))], spec_for("+z"), iso_value=100.0)
    assert (out["flags"] == MISS).all() and (out["steps"] == NSTEPS).all()
    for k in ("rgba", "depth", "label", "pick", "normal"):
        assert not out[k].any(), k
    # outside the block nothing runs: a frame wider than the volume
    spec = spec_for("+z")
    spec.ortho_size = (64.0, 64.0)
    wide = iso_twin([ring(np.full((N, N, N), 200, np.uint8))], spec.matrices(), (f32(N),) * 3, material(), FRAME, FRAME,
                    dict(SHADE, iso_value=100.0))
    assert (wide["flags"] == DISCARD).sum() == FRAME * FRAME - 64 and (wide["flags"] == HIT).sum() == 64
    assert not wide["steps"][wide["flags"] == DISCARD].any()


def test_a_level_at_or_below_every_value_hits_the_first_sample_without_refinement():
    for level in (100.0, 0.0, -5.0, float("-inf")):
        out = run([ring(np.full((N, N, N), 100, np.uint8))], spec_for("+z"), iso_value=level, refine=8)
        assert (out["flags"] == HIT).all() and (out["steps"] == 1).all() and (out["iter"] == 0.0).all()
    out = run([ring(np.full((N, N, N), 100, np.uint8))], spec_for("+z"), iso_value=float("inf"))
    assert (out["flags"] == MISS).all()


def test_refinement_takes_the_first_sub_sample_at_the_level():
    rings = [ring(step_along_x(10))]
    # sample 35 at x = 9.912, 36 at 10.195; sub-samples 35.25 at 9.982 (below), 35.5 at 10.053 (the first at the level)
    for refine, want in ((0, 36.0), (1, 36.0), (2, 35.5), (4, 35.5), (8, 35.375), (16, 35.3125)):
        assert 10.0 <= want * N / NSTEPS < 10.0 + N / NSTEPS / max(refine, 1)
        out = run(rings, spec_for("+x"), iso_value=100.0, refine=refine)
        assert (out["iter"] == f32(want)).all(), (refine, np.unique(out["iter"]))
        assert (out["steps"] == 37).all()                    # the coarse count does not depend on refine
    # a linear search: a one-voxel wall between the samples 35 and 36 is found by the sub-sample that lands in it, and
    # the coarse candidate (a later sample, in the dense half behind) is not what is reported
    d = step_along_x(12)
    d[:, :, 10] = 200
    d[:, :, 11] = 0
    out = run([ring(d)], spec_for("+x"), iso_value=100.0, refine=4)
    assert (out["iter"] == f32(35.5)).all() and (out["steps"] == 37).all()


def test_a_zero_gradient_falls_back_to_the_view_direction():
    d = np.zeros((N, N, N), np.uint8)
    d[:, :, 10] = 200                                        # a one-voxel sheet: both x taps are 0, y and z taps are equal
    out = run([ring(d)], spec_for(angled), iso_value=100.0)
    y = ((out["pick"] >> np.uint64(34)) & np.uint64(0x3FFF)).astype(np.float64) / 16383.0 * N
    hit = (out["flags"] == HIT) & (y > 2.0) & (y < N - 2.0)  # (at the block's y faces one y tap leaves the volume)
    assert hit.sum() > 60
    assert np.abs(out["normal"][hit] - np.array([-0.6, -0.8, 0.0])).max() < 1e-6
    t, s = 0.25 + 0.5, 0.125                                  # n = v: |n.l| = |n.h| = 1
    assert np.abs(out["rgba"][hit] - np.array([0.5 * t + s, t + s, 0.25 * t + s, 0.75])).max() < 2e-6
    # a NaN gradient (float ring) falls back too
    e = d.astype(f32)
    e[:, :, 11] = np.inf
    e[:, :, 9] = np.inf                                      # inf - inf
    out = iso_twin([dict(ring(d), density=e)], spec_for("+x").matrices(), (f32(N),) * 3, material(), FRAME, FRAME,
                   dict(SHADE, iso_value=100.0))
    assert np.array_equal(out["normal"][out["flags"] == HIT], np.broadcast_to(np.array([-1.0, 0.0, 0.0], f32), (FRAME * FRAME, 3)))


def test_anisotropic_scale_tilts_the_normal_by_the_inverse_transpose():
    zz, yy, xx = np.meshgrid(*[np.arange(N)] * 3, indexing="ij")
    d = np.where(xx + yy >= 32, 200, 0).astype(np.uint8)     # the first dense voxel along +x has x + y == 32: g = (200, 200, 0)
    out = run([ring(d)], spec_for("+x"), iso_value=100.0)
    assert (out["flags"] == HIT).all()
    assert np.abs(out["normal"] - np.array([-1.0, -1.0, 0.0]) / math.sqrt(2.0)).max() < 1e-6
    # world scale (1, 2, 1): the surface x + y/2 = const has the normal (1, 1/2, 0), not (1, 2, 0)
    out = run([ring(d)], spec_for("+x", world_scale=(1.0, 2.0, 1.0)), iso_value=100.0)
    assert (out["flags"] == HIT).all()
    assert np.abs(out["normal"] - np.array([-2.0, -1.0, 0.0]) / math.sqrt(5.0)).max() < 1e-6
    ndl = 2.0 / math.sqrt(5.0)                               # v = l = (-1, 0, 0)
    assert np.abs(out["rgba"][..., 1] - ((0.25 + 0.5 * ndl) + 0.125 * ndl ** 4)).max() < 2e-6


def test_a_hit_on_a_lod_1_voxel_takes_lod_1_tap_spacing_and_labels():
    fine = np.zeros((N, N, N), np.uint8)                     # LOD 0 holds z < 8 only, and is empty
    coarse = np.zeros((16, 16, 16), np.uint8)                # LOD 1 voxels are 2 data voxels wide
    coarse[6:] = 120
    coarse[6:, :, 7:9] = 200                                 # a ridge on the LOD-1 columns 7 and 8, mirror-symmetric in x
    labels = np.full((16, 16, 16), 9, np.uint32)
    out = run([ring(fine, z_range=(0, 8)), ring(coarse, labels, scale=0.5)], spec_for("+z"), iso_value=100.0,
              color_by_label=True)
    assert (out["flags"] == HIT).all() and (out["label"] == 9).all()
    # samples at z = i * 32 / 113: the first in LOD-1 voxel 6 (z in [12, 14)) is sample 43 (12.18)
    assert (out["steps"] == 44).all()
    # The 16 pixel columns look down the data columns x = 8.5 .. 23.5 (in one screen order or the other: the field is
    # symmetric about x = 16).  Taps are two data voxels apart (one LOD-1 voxel), so over the ridge (LOD-1 voxels 7, 8:
    # the columns 6 .. 9) the x neighbours are 120 and 200 and the z neighbours 0 and 200: g = (+-40, 0, 100); over the
    # voxels 6 and 9 next to it (columns 4, 5, 10, 11; value 120) they are 120 and 200, 0 and 120: g = (+-40, 0, 60);
    # further out the x neighbours are equal.  Taps one data voxel apart would find no x gradient at x = 13.5 and
    # 15.5 (both taps inside one LOD-1 voxel or inside the ridge).
    nx, nz = out["normal"][0, :, 0], out["normal"][0, :, 2]
    assert (out["normal"] == out["normal"][0]).all()                                     # the rows are alike
    for cols, gz in ((np.r_[6:10], 100.0), (np.r_[4:6, 10:12], 60.0)):
        assert np.abs(np.abs(nx[cols]) - 40.0 / math.hypot(40.0, gz)).max() < 1e-6
        assert np.abs(nz[cols] + gz / math.hypot(40.0, gz)).max() < 1e-6
    assert (np.sign(nx[4:8]) == -np.sign(nx[8:12])).all() and len(set(np.sign(nx[4:8]))) == 1
    outer = np.r_[0:4, 12:16]
    assert np.array_equal(out["normal"][:, outer], np.broadcast_to(np.array([0.0, 0.0, -1.0], f32), (FRAME, 8, 3)))
    assert (out["normal"][:, :, 1] == 0.0).all()
    # colors[9 % 2] = (h 0.25, s 1): hsv_to_rgb(0.25, 1, 1) = (0.5, 1, 0); v = l = h = (0, 0, -1)
    ndl = 100.0 / math.hypot(40.0, 100.0)
    t, s = 0.25 + 0.5 * ndl, 0.125 * ndl ** 4
    assert np.abs(out["rgba"][:, 6:10] - np.array([0.5 * t + s, t + s, s, 0.75])).max() < 2e-6


# ---- the material ---------------------------------------------------------------------------------------------------
def test_material_iso_mode_and_its_properties():
    m = SubVolumeMaterial(0.5)
    assert "iso" in SubVolumeMaterial.RENDER_MODES and m.render_mode == "lmip"
    assert (m.iso_value, m.iso_refine, m.iso_color, m.light_direction) == (0.5, 4, tuple(float(f32(c)) for c in (0.8, 0.8, 0.8)), None)
    assert (m.ambient, m.diffuse, m.specular, m.shininess_log2) == (float(f32(0.2)), float(f32(0.7)), float(f32(0.3)), 5)
    for name, value in (("render_mode", "iso"), ("iso_value", 120.0), ("iso_color", (0.1, 0.2, 0.3)), ("iso_refine", 16),
                        ("ambient", 0.0), ("diffuse", 2.0), ("specular", 0.5), ("shininess_log2", 10),
                        ("light_direction", (0.0, 3.0, 4.0)), ("light_direction", None), ("color_by_label", True),
                        ("iso_value", float("inf")), ("iso_refine", 0), ("shininess_log2", 0)):
        v = m._version
        setattr(m, name, value)
        assert m._version > v, name
    m.light_direction = (0.0, 3.0, 4.0)
    assert np.allclose(m.light_direction, (0.0, 0.6, 0.8)) and m.render_mode == "iso"
    bad = [("iso_value", float("nan")), ("iso_value", "1"), ("iso_color", (0.1, 0.2)), ("iso_color", (0.1, 1.5, 0.2)),
           ("iso_color", (0.1, float("nan"), 0.2)), ("iso_color", "red"), ("iso_refine", -1), ("iso_refine", 17),
           ("iso_refine", 2.5), ("ambient", -0.1), ("diffuse", float("inf")), ("specular", float("nan")), ("specular", "x"),
           ("shininess_log2", 11), ("shininess_log2", -1), ("shininess_log2", 1.5), ("light_direction", (0.0, 0.0, 0.0)),
           ("light_direction", (1.0, 2.0)), ("light_direction", (float("nan"), 0.0, 1.0)), ("light_direction", "up"),
           ("render_mode", "fading")]
    for name, value in bad:
        v = m._version
        with pytest.raises(ValueError):
            setattr(m, name, value)
        assert m._version == v, name
    # the LMIP uniforms are sent unchanged in iso mode (svr_iso does not read them)
    assert m.lmip_uniforms() == (0.5, 0.5, 10)


def test_iso_result_extends_render_result_without_touching_it():
    import dataclasses

    assert [f.name for f in dataclasses.fields(RenderResult)] == ["rgba", "depth", "label", "flags", "steps", "pick"]
    assert [f.name for f in dataclasses.fields(IsoResult)][6:] == ["normal", "skip_counters"]
    r = IsoResult(1, 2, 3, 4, 5)
    assert isinstance(r, RenderResult) and r.pick is None and r.normal is None and r.skip_counters is None


def test_header_declares_svr_iso_within_abi_9():
    import ctypes as C

    header = open(os.path.join(ROOT, "include", "svr.h")).read()
    assert re.search(r"#define SVR_ABI_VERSION 9\b", header)
    assert re.search(r"int\s+svr_iso\(svr_ctx\* ctx, const svr_camera\* cam, const svr_frame\* frame, "
                     r"const svr_iso_params\* params,\s+const svr_outputs\* out, void\* stream\);", header)
    body = re.search(r"typedef struct svr_iso_params \{(.*?)\} svr_iso_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [n for n, _ in _native.IsoParams._fields_]
    assert C.sizeof(_native.IsoParams) == 80 and _native.IsoParams.normal.offset == 64
    assert "svr_iso" in _native.SIGNATURES
    assert int(re.search(r"#define SVR_ISO_MAX_REFINE (\d+)", header).group(1)) == _native.ISO_MAX_REFINE
    assert int(re.search(r"#define SVR_ISO_MAX_SHININESS_LOG2 (\d+)", header).group(1)) == _native.ISO_MAX_SHININESS_LOG2


def test_nan_and_infinite_samples_against_negative_zero_and_infinite_levels():
    """s >= iso_value on the signed sample, IEEE: a NaN sample is passed over at every level (-inf included), +inf
    reaches every level, -inf only the level -inf; an all-NaN block is a MISS that runs every step."""
    spec = spec_for("+z")
    first_x = int(np.ceil(10 * NSTEPS / N))                       # the first sample in voxel 10 along the ray
    for fill, dense, level, want in (
            (np.nan, 5.0, -40.0, "late"), (np.nan, 5.0, 0.0, "late"), (np.nan, 5.0, float("-inf"), "late"),
            (np.nan, -np.inf, float("-inf"), "late"), (np.nan, -np.inf, -1e30, "miss"), (np.nan, np.inf, 3e38, "late"),
            (-np.inf, np.nan, float("-inf"), "first"), (-50.0, np.nan, -40.0, "miss"), (np.nan, np.nan, float("-inf"), "miss"),
            (-0.0, 7.0, 0.0, "first")):
        d = np.full((N, N, N), fill, np.float32)
        d[10:] = dense                                            # [z, y, x]: the +z rays meet `dense` from voxel 10 on
        out = run([ring(d)], spec, iso_value=level, refine=0)
        what = (fill, dense, level)
        if want == "miss":
            assert (out["flags"] == MISS).all() and (out["steps"] == NSTEPS).all(), what
        else:
            assert (out["flags"] == HIT).all(), what
            assert (out["steps"] == (1 if want == "first" else first_x + 1)).all(), (what, out["steps"][0, 0], first_x)
        assert np.isfinite(out["rgba"]).all() and np.isfinite(out["normal"]).all(), what      # n falls back to v


def test_a_refinement_sample_that_is_nan_is_passed_over():
    d = np.zeros((N, N, N), np.float32)
    d[10:] = 200.0
    spec = spec_for("+z")
    plain = run([ring(d)], spec, iso_value=100.0, refine=4)
    d[10] = np.nan                                                # the layer the refinement would have found first
    d[9] = 0.0
    out = run([ring(d)], spec, iso_value=100.0, refine=4)
    assert (out["flags"] == HIT).all() and (plain["flags"] == HIT).all()
    # the coarse candidate moves to the first sample in voxel 11 and the sub-samples before it (in the NaN layer) fail
    first_11 = int(np.ceil(11 * NSTEPS / N))
    assert (out["steps"] == first_11 + 1).all() and (out["iter"] == np.float32(first_11)).all(), (out["steps"][0, 0], out["iter"][0, 0])
    assert (plain["iter"] < out["iter"]).all()
