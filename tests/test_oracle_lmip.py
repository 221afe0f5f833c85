"""The shader oracle (oracle/lmip_oracle.c): committed golden vectors, agreement with the independent
numpy restatement, and hand-derived known answers.  Render parity is *unpinned* by the reference (it
holds no rendered fixture); these tests pin the restatement itself."""
import os
import sys

import numpy as np
import pytest

from oracle import lmip, lmip_numpy
from sub_volume_renderer_amd import testing

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden  # noqa: E402

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_golden.npz"))


@pytest.mark.parametrize("name", ["demo", "k1", "k2"])
def test_oracle_reproduces_committed_golden(name):
    r = lmip.render_spec(make_golden.specs()[name], nthreads=2)
    for plane in ("label", "flags", "steps"):
        np.testing.assert_array_equal(getattr(r, plane), GOLD[f"{name}_{plane}"])
    np.testing.assert_allclose(r.rgba, GOLD[f"{name}_rgba"], rtol=0, atol=1e-6)      # libm pow/exp may differ by an ulp
    np.testing.assert_allclose(r.depth, GOLD[f"{name}_depth"], rtol=0, atol=1e-6)
    assert (GOLD[f"{name}_flags"] == 2).sum() > 0


@pytest.mark.parametrize("name", ["demo", "k1", "k2"])
def test_two_independent_restatements_agree(name):
    spec = make_golden.specs()[name]
    a = lmip.render_spec(spec, nthreads=2)
    b = lmip_numpy.render_spec(spec)
    np.testing.assert_array_equal(a.flags, b["flags"])
    np.testing.assert_array_equal(a.steps, b["steps"])
    np.testing.assert_array_equal(a.label, b["label"])
    np.testing.assert_allclose(a.rgba, b["rgba"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(a.depth, b["depth"], rtol=0, atol=2e-6)


def _uniform_scene(value, threshold):
    data = np.full((16, 16, 16), value, np.float32)
    seg = np.full((16, 16, 16), 2, np.uint32)
    spec = testing.synthetic_spec(16, 40, 30, pairs=[(data, seg)], chunk_shapes=[(4, 4, 4)], ring_shapes=[(4, 4, 4)])
    spec.material = dict(lmip_threshold=threshold, fog_density=0.25, fog_color=(0.2, 0.4, 0.6),
                         colors=[(0.0, 1.0, 1.0), (0.5, 1.0, 1.0), (1.0 / 3.0, 1.0, 1.0)], opacity=0.9)
    spec.centers = [((7.5, 7.5, 7.5), [(16, 16, 16)])]
    return spec


def test_all_zero_volume_is_black_and_opaque():
    """The reference's (stale) render test idea: an all-zero volume renders black (tests/basic_volume/
    test_volume_texture_update.py:17-38); fs_main.wgsl:93-98 gives (0,0,0,1), depth 0."""
    r = lmip.render_spec(_uniform_scene(0.0, 0.5))
    frag = r.flags != 0
    assert frag.sum() > 0 and (r.flags == 2).sum() == 0
    assert np.all(r.rgba[frag] == np.array([0, 0, 0, 1], np.float32))
    assert np.all(r.rgba[~frag] == 0) and np.all(r.depth == 0)
    assert np.all(r.steps[~frag] == 0) and np.all(r.steps[frag] >= 1)


def test_uniform_one_volume_known_colour():
    """Every ray hits at iteration 0 (value 1 >= 0.5); with lmip_max_samples = 10 and no fall-off it
    stops after min(nsteps, 11) samples.  v = 1 -> srgb2physical(1) = 1; label 2 -> hue 1/3 -> pure
    green; offset = 0 -> fog factor 1 -> rgba = (0, 1, 0, opacity)."""
    r = lmip.render_spec(_uniform_scene(1.0, 0.5))
    hit = r.flags == 2
    # rays grazing the far faces sample exactly at coord == size (voxel index 16: outside every ROI, value 0)
    assert hit.sum() > 0 and (r.flags == 1).sum() < 0.05 * hit.sum()
    assert np.all(r.steps[r.flags == 1] <= 2)
    want = np.tile(np.array([0, 1, 0, 0.9], np.float32), (hit.sum(), 1))
    np.testing.assert_allclose(r.rgba[hit], want, atol=5e-3)          # grazing rays hit at iteration 1: a trace of fog
    exact = np.all(np.abs(r.rgba[hit] - want) <= 1e-6, axis=1)
    assert exact.mean() > 0.5         # rays entering through a low face: hit at iteration 0, offset 0, no fog at all
    assert np.all(r.label[hit] == 2)
    full = lmip.render_spec(_uniform_scene(1.0, float("inf")))        # threshold never reached
    # raycast.wgsl:43,47,58: 1 + max_samples samples from the first hit; rays entering through a high face
    # take their first sample at coord == size (outside every ROI), so they run one step more
    extra = r.steps[hit].astype(int) - np.minimum(full.steps[hit], 11).astype(int)
    assert set(np.unique(extra)) <= {0, 1}


def test_lod_fallthrough_first_roi_wins_even_if_zero():
    """sample_vol.wgsl:51-63: the first LOD whose ROI holds the voxel wins even when its value is 0."""
    n = 16
    d0 = np.zeros((n, n, n), np.float32)                 # LOD 0: all zero, loaded everywhere
    d1 = np.ones((n // 2,) * 3, np.float32)              # LOD 1: all one
    s0 = np.zeros(d0.shape, np.uint32)
    s1 = np.ones(d1.shape, np.uint32)
    spec = testing.synthetic_spec(n, 32, 24, pairs=[(d0, s0), (d1, s1)], chunk_shapes=[(4, 4, 4), (2, 2, 2)],
                                  ring_shapes=[(4, 4, 4), (4, 4, 4)])
    spec.material.update(lmip_threshold=0.5, clim=(0, 1))
    spec.centers = [((7.5, 7.5, 7.5), [(16, 16, 16), (8, 8, 8)])]
    r = lmip.render_spec(spec)
    assert (r.flags == 2).sum() == 0                     # LOD 0 covers everything with zeros
    spec.centers = [((7.5, 7.5, 7.5), [(8, 8, 8), (8, 8, 8)])]       # LOD 0 only in the middle
    r = lmip.render_spec(spec)
    assert (r.flags == 2).sum() > 0 and set(np.unique(r.label[r.flags == 2])) == {1}


def test_region_rendering_matches_full_frame():
    from sub_volume_renderer_amd import FrameRegion

    spec = make_golden.specs()["k1"]
    full = lmip.render_spec(spec)
    tile = lmip.render_spec(spec, region=FrameRegion.tile(16, 8, 40, 24))
    np.testing.assert_array_equal(tile.rgba, full.rgba[8:32, 16:56])
    st = FrameRegion.stripes(80, 48, 1, 3, band_h=8)
    r = lmip.render_spec(spec, region=st)
    for row in range(st.out_h):
        y = st.y0 + (row // 8) * st.band_pitch + row % 8
        if y < 48:
            np.testing.assert_array_equal(r.label[row], full.label[y])
        else:
            assert np.all(r.flags[row] == 0)


def test_pick_word_layout_and_restatements_agree():
    """fs_main.wgsl:89-92 (`write_pick`): 20 bits of wobject id, then 14 bits each of u32(coord * 16383)
    for x, y, z, at running bit offsets of a 64-bit word (pygfx pick_pack, restated; parity unpinned)."""
    spec = make_golden.specs()["k1"]
    a = lmip.render_spec(spec, nthreads=2, pick_id=0x12345)
    b = lmip_numpy.render_spec(spec, pick_id=0x12345)
    np.testing.assert_array_equal(a.pick, b["pick"])
    hit = a.flags == 2
    assert hit.sum() > 0 and np.all(a.pick[~hit] == 0)
    w = a.pick[hit]
    assert np.all((w & np.uint64(0xFFFFF)) == np.uint64(0x12345))
    for shift in (20, 34, 48):
        f = (w >> np.uint64(shift)) & np.uint64(0x3FFF)
        assert f.max() <= 16383 and f.min() >= 0 and len(np.unique(f)) > 4      # coordinates vary over the frame
    assert np.all((w >> np.uint64(62)) == 0)
    # an id wider than 20 bits is clipped, as pick_pack clips every field to its width
    c = lmip.render_spec(spec, nthreads=2, pick_id=0xFFFFFFF)
    assert np.all((c.pick[hit] & np.uint64(0xFFFFF)) == np.uint64(0xFFFFF))
    np.testing.assert_array_equal(c.pick[hit] >> np.uint64(20), w >> np.uint64(20))


# ---- clipping planes (fs_main.wgsl:8: pygfx.clipping_planes.wgsl, restated — assumption A6) -----------------------
def _back_face_world_x(spec):
    """World x of the point where each pixel's ray leaves the proxy box, in float64 (independent of both
    restatements' f32 chains): NaN where the ray misses the box."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    n2d = M["world_inv"] @ M["cam_inv"] @ M["proj_inv"]
    W, H = spec.width, spec.height
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = 2 * (ii + 0.5) / W - 1, 1 - 2 * (jj + 0.5) / H
    def unproject(z):
        v = np.einsum("rc,chw->rhw", n2d, np.stack([px, py, np.full_like(px, z), np.ones_like(px)]))
        return v[:3] / v[3]
    near, far = unproject(-1.0), unproject(1.0)
    ray = (far - near) / np.linalg.norm(far - near, axis=0)
    size = np.array(spec.pairs[0][0].shape[::-1], np.float64)[:, None, None]
    with np.errstate(all="ignore"):
        t1, t2 = (-0.5 - near) / ray, (size - 0.5 - near) / ray
    t_exit, t_enter = np.maximum(t1, t2).min(axis=0), np.minimum(t1, t2).max(axis=0)
    back = near + ray * t_exit
    wx = M["world"][0, 0] * back[0] + M["world"][0, 1] * back[1] + M["world"][0, 2] * back[2] + M["world"][0, 3]
    return np.where(t_enter <= t_exit, wx, np.nan)


@pytest.mark.parametrize("mode", ["ANY", "ALL"])
def test_clipping_planes_discard_rays_by_their_back_face_position(mode):
    spec = make_golden.specs()["k1"]
    base = lmip.render_spec(spec, nthreads=2)
    n = spec.pairs[0][0].shape[0]
    # plane 1: x >= n/2 is kept; plane 2: everything kept (ANY) / nothing clipped by it alone
    spec.material = dict(spec.material, clipping_planes=[(1.0, 0.0, 0.0, n / 2.0), (0.0, 1.0, 0.0, -1e6)], clipping_mode=mode)
    a = lmip.render_spec(spec, nthreads=2)
    b = lmip_numpy.render_spec(spec)
    np.testing.assert_array_equal(a.flags, b["flags"])
    np.testing.assert_array_equal(a.label, b["label"])
    np.testing.assert_array_equal(a.steps, b["steps"])
    wx = _back_face_world_x(spec)
    margin = 1e-3 * n
    if mode == "ANY":
        assert np.all(a.flags[wx < n / 2.0 - margin] == 0)                      # behind plane 1: discarded
        keep = wx > n / 2.0 + margin
        assert keep.sum() > 100 and (base.flags[keep] != 0).sum() > 100
        np.testing.assert_array_equal(a.flags[keep], base.flags[keep])            # in front of both: untouched
        np.testing.assert_array_equal(a.rgba[keep], base.rgba[keep])
        assert (a.flags != base.flags).sum() > 100
    else:
        np.testing.assert_array_equal(a.flags, base.flags)                       # no point is behind BOTH planes


def test_no_clipping_planes_is_the_default_and_changes_nothing():
    spec = make_golden.specs()["demo"]
    a = lmip.render_spec(spec, nthreads=2)
    spec.material = dict(spec.material, clipping_planes=[], clipping_mode="ALL")
    b = lmip.render_spec(spec, nthreads=2)
    for plane in ("flags", "label", "steps", "rgba", "depth"):
        np.testing.assert_array_equal(getattr(a, plane), getattr(b, plane))


# ---- MIP render mode (FUTURE.md:97-120) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k1", "k2"])
def test_mip_mode_through_the_lmip_machine_equals_mip_stated_directly(name):
    spec = make_golden.specs()[name]
    spec.material = dict(spec.material, render_mode="mip")
    a = lmip.render_spec(spec, nthreads=2)                 # LMIP state machine with MIP parameters (C)
    b = lmip_numpy.render_spec(spec)                       # running maximum over the whole ray (numpy)
    np.testing.assert_array_equal(a.flags, b["flags"])
    np.testing.assert_array_equal(a.steps, b["steps"])
    np.testing.assert_array_equal(a.label, b["label"])
    np.testing.assert_allclose(a.rgba, b["rgba"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(a.depth, b["depth"], rtol=0, atol=2e-6)
    assert (a.flags == 1).sum() == 0 and (a.flags == 2).sum() > 500      # every fragment yields its maximum
    full = dict(spec.material, render_mode="lmip", lmip_threshold=float("inf"))
    spec.material = full
    np.testing.assert_array_equal(a.steps, lmip.render_spec(spec, nthreads=2).steps)      # MIP walks the whole ray


# ---- weighted-average render mode (named in FUTURE.md:97-109, defined by this project: include/svr.h) ----------------
@pytest.mark.parametrize("falloff", [0.0, 0.5, 3.0])
@pytest.mark.parametrize("name", ["k1", "k2"])
def test_weighted_average_two_restatements_agree(name, falloff):
    spec = make_golden.specs()[name]
    spec.material = dict(spec.material, render_mode="weighted_average", weight_falloff=falloff)
    a = lmip.render_spec(spec, nthreads=2)
    b = lmip_numpy.render_spec(spec)
    np.testing.assert_array_equal(a.flags, b["flags"])
    np.testing.assert_array_equal(a.steps, b["steps"])
    np.testing.assert_array_equal(a.label, b["label"])
    np.testing.assert_allclose(a.rgba, b["rgba"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(a.depth, b["depth"], rtol=0, atol=2e-6)
    assert (a.flags == 2).sum() > 500
    plain = make_golden.specs()[name]
    plain.material = dict(plain.material, lmip_threshold=float("inf"))            # LMIP that never triggers: the whole ray
    whole = lmip.render_spec(plain, nthreads=2)
    if falloff <= 0.5:                     # range 1 / falloff >= 2 volume edges: longer than any ray, nothing is cut
        np.testing.assert_array_equal(a.steps, whole.steps)
    else:                                  # range 1/3 of an edge: long rays stop early
        assert np.all(a.steps <= whole.steps) and (a.steps < whole.steps).sum() > 500


def test_weighted_average_known_answers():
    """Uniform volume of ones: sum(w * 1) == sum(w) bit for bit, so the mean is exactly 1 whatever the weights;
    the largest contribution is the first sample's (w = 1, later ones weigh less) -> offset 0 -> no fog:
    the same pure green as the LMIP known answer.  All zeros: nothing contributes -> a miss, black and opaque.
    Range shorter than one step: exactly one sample per ray."""
    spec = _uniform_scene(1.0, 0.5)
    spec.material.update(render_mode="weighted_average", weight_falloff=0.5)
    r = lmip.render_spec(spec)
    hit = r.flags == 2
    assert hit.sum() > 0 and (r.flags == 1).sum() < 0.05 * hit.sum()
    want = np.tile(np.array([0, 1, 0, 0.9], np.float32), (hit.sum(), 1))
    # rays entering through a high face take their first sample outside every ROI (value 0): the mean is then a
    # little below 1 and the strongest sample is the second one
    exact = np.all(np.abs(r.rgba[hit] - want) <= 1e-6, axis=1)
    assert exact.mean() > 0.5
    assert np.all(r.rgba[hit][:, 1] <= 1.0 + 1e-6) and np.all(r.rgba[hit][:, [0, 2]] <= 5e-3)      # never brighter than the data
    assert np.all(r.label[hit] == 2)

    zero = _uniform_scene(0.0, 0.5)
    zero.material.update(render_mode="weighted_average")
    z = lmip.render_spec(zero)
    frag = z.flags != 0
    assert frag.sum() > 0 and (z.flags == 2).sum() == 0
    assert np.all(z.rgba[frag] == np.array([0, 0, 0, 1], np.float32))

    spec.material.update(weight_falloff=1.0e4)            # range 1e-4 of an edge: the second sample already weighs nothing
    one = lmip.render_spec(spec)
    assert np.all(one.steps[one.flags != 0] == 1)


def test_weighted_average_prefers_near_structures():
    """Two bright slabs of equal value along z, camera on the -z side... the pixel is shown at the slab nearer to
    the ray's entry (larger weight), and a larger fall-off moves the mean towards the near part of the ray."""
    n = 32
    d = np.zeros((n, n, n), np.float32)
    d[4:8] = 1.0                                           # z in [4, 8)
    d[24:28] = 1.0                                         # z in [24, 28)
    seg = np.zeros(d.shape, np.uint32)
    seg[4:8], seg[24:28] = 1, 2
    spec = testing.synthetic_spec(n, 48, 36, pairs=[(d, seg)], chunk_shapes=[(8, 8, 8)], ring_shapes=[(4, 4, 4)])
    spec.centers = [((15.5, 15.5, 15.5), [(n, n, n)])]
    spec.material = dict(lmip_threshold=0.5, fog_density=0.0, colors=[(0.0, 0.0, 1.0)], clim=(0.0, 1.0),
                         render_mode="weighted_average", weight_falloff=0.5)
    spec.cam_position, spec.cam_target = (15.5, 15.5, -60.0), (15.5, 15.5, 15.5)
    near_first = lmip.render_spec(spec)
    hit = near_first.flags == 2
    centre = (slice(14, 22), slice(20, 28))                # rays through both slabs
    assert np.all(near_first.label[centre] == 1)
    spec.cam_position = (15.5, 15.5, 91.0)
    far_first = lmip.render_spec(spec)
    assert np.all(far_first.label[centre] == 2)
    # grey value = the mean itself (saturation 0, clim 0..1, no fog; "linear" so that no transfer curve is applied)
    spec.colorspace = "linear"
    lo = lmip.render_spec(spec).rgba[centre][..., 0]
    spec.material.update(weight_falloff=1.0)
    hi = lmip.render_spec(spec).rgba[centre][..., 0]
    assert np.all((lo > 0.05) & (lo < 0.6))                # 8 of ~32 voxels along the ray are bright
    assert hit.sum() > 100 and not np.allclose(lo, hi)


@pytest.mark.parametrize("offset", [(0, 0, 0), (0, 5, 0), (0, 0, 5), (0, -7, 3), (6, 4, -9)])
def test_single_voxel_lands_where_the_camera_conventions_say(offset):
    """End-to-end known answer that does not go through matrices shared with the product: one bright voxel, a camera
    on the +x axis; where it must appear on screen follows from the conventions alone (testing.single_voxel_spec).
    A flipped y, a mirrored x, a wrong field-of-view rule or a half-pixel shift would move it."""
    r = lmip.render_spec(testing.single_voxel_spec(offset))
    rows, cols = np.nonzero(r.flags == 2)
    assert rows.size >= 1
    want_row, want_col = testing.expected_single_voxel_pixel(offset)
    # the voxel is one unit wide, a pixel 1.02 units at the centre plane: the hits form a blob of <= 3 x 3 pixels around it
    assert abs(rows.mean() - want_row) <= 0.75 and abs(cols.mean() - want_col) <= 0.75, (rows, cols, want_row, want_col)
    assert rows.max() - rows.min() <= 2 and cols.max() - cols.min() <= 2
    assert np.all(r.label[r.flags == 2] == 7)
    # depth: the voxel's centre through proj * cam * world as fs_main.wgsl:61-72 writes it: (coord - 0.5) is a NORMALISED
    # coordinate there, so the depth belongs to a point next to the volume's origin corner: only its range is checked here
    assert np.all((r.depth[r.flags == 2] > 0) & (r.depth[r.flags == 2] < 1))


# ---- orthographic cameras: parallel rays, exact-zero ray components, pixel centres on faces ------------------------
import ortho_scenes as ortho  # noqa: E402


def _restatements_agree(spec, pick_id=0x2A):
    a = lmip.render_spec(spec, nthreads=2, pick_id=pick_id)
    b = lmip_numpy.render_spec(spec, pick_id=pick_id)
    for plane in ("flags", "steps", "label", "pick", "depth"):
        np.testing.assert_array_equal(getattr(a, plane), b[plane], err_msg=plane)
    np.testing.assert_allclose(a.rgba, b["rgba"], rtol=0, atol=2e-6)      # libm pow / exp may differ by an ulp
    return a


def _ortho_pairs(n=32, nlod=2):
    from sub_volume_renderer_amd import synth

    return [synth.volume(n, k, 64) for k in range(nlod)]


def _ortho_base(width=64, height=64, **material):
    # LOD 0's window (16^3 around a point off the centre) wraps around its ring and ends inside the view; LOD 1 covers
    # the rest
    return ortho.base_spec(_ortho_pairs(), [(8, 8, 8), (4, 4, 4)], [(2, 2, 2), (4, 4, 4)], width, height,
                           centre=(13.0, 18.0, 11.0), **{"lmip_threshold": 120.0, **material})


@pytest.mark.parametrize("view", ["+x", "-x", "+y", "-y", "+z", "-z"])
@pytest.mark.parametrize("ppv,face", [(1, False), (1, True), (2, True)], ids=["centres", "faces", "faces-2ppv"])
def test_orthographic_axis_views_restatements_agree(view, ppv, face):
    spec = ortho.axis_view(_ortho_base(64 * ppv, 64 * ppv), view, ppv=ppv, face=face)   # 64 voxels wide: past both box faces
    a_, s_ = ortho.AXES[view]
    # two of the three direction components are exactly zero in the matrices both sides receive
    d = ortho.direction_column(spec)
    assert np.count_nonzero(d) == 1 and np.sign(d[a_]) == s_, d
    near, ray = ortho.pixel_rays(spec)
    assert np.all(np.delete(ray, a_, axis=0) == 0.0)
    others = [k for k in range(3) if k != a_]
    size = ortho.size_xyz(spec)
    on_face = np.zeros(near.shape[1:], bool)
    for k in others:
        on_face |= ortho.face_distance(near[k]) == 0.0
    if face:
        assert on_face.sum() >= spec.width * spec.height // (2 if ppv == 2 else 1)
        for k in others:                                   # ... the box faces among them: the 0/0 rays
            assert np.any(near[k] == -0.5) and np.any(near[k] == size[k] - 0.5)
    else:
        assert not on_face.any()
    r = _restatements_agree(spec)
    assert (r.flags == 2).sum() > 100 and (r.flags == 0).sum() > 100


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_orthographic_view_rotated_about_one_axis(axis):
    """An exact rotation about one axis (3-4-5 triangle) set through rotation_matrix: about x or y the direction keeps
    one exact zero and the two others are oblique; about z (the view axis) the screen axes are rolled."""
    spec = _ortho_base(64, 32)
    spec.projection, spec.ortho_size = "orthographic", (48.0, 24.0)
    c, s = 0.6, 0.8
    R = np.eye(3)
    i, j = [k for k in range(3) if k != axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    cam = spec.camera()
    centre = np.array([15.5, 15.5, 15.5])
    back = R @ np.array([0.0, 0.0, 1.0])                  # the camera's local +z (it looks down local -z)
    cam.world.position = tuple(centre + 60.0 * back)
    cam.world.rotation_matrix = R
    spec.depth_range = (1.0, 200.0)
    spec.camera = lambda cam=cam: cam                     # the hand-set pose, for the product and the oracle alike
    d = ortho.direction_column(spec)
    if axis == 2:                                         # a roll about the view axis: both screen axes oblique,
        assert np.count_nonzero(d) == 1 and d[2] < 0, d   # the direction still exactly -z
    else:
        assert np.count_nonzero(d) == 2 and d[axis] == 0.0, d
    r = _restatements_agree(spec)
    assert (r.flags == 2).sum() > 100


def test_orthographic_oblique_view():
    spec = _ortho_base(64, 48)
    spec.projection, spec.ortho_size = "orthographic", (50.0, 37.5)
    spec.cam_position, spec.cam_target = (70.0, -35.0, 52.0), (15.5, 15.5, 15.5)
    spec.depth_range = (1.0, 200.0)
    assert np.all(ortho.direction_column(spec) != 0.0)
    r = _restatements_agree(spec)
    assert (r.flags == 2).sum() > 100 and (r.flags == 0).sum() > 100


@pytest.mark.parametrize("view", ["-z", "+y", "oblique"])
def test_orthographic_camera_inside_with_the_near_plane_behind_it(view):
    spec = _ortho_base(64, 64)
    eye = np.array([14.0, 17.0, 12.0])
    d = {"-z": (0, 0, -1.0), "+y": (0, 1.0, 0), "oblique": (0.5, -0.3, 0.8)}[view]
    spec.projection, spec.ortho_size = "orthographic", (24.0, 24.0)
    spec.cam_position, spec.cam_target = tuple(eye), tuple(eye + np.array(d))
    spec.depth_range = (-6.0, 40.0)                       # the near plane 6 units behind the camera, inside the volume
    M = spec.matrices()
    P = np.asarray(M["proj"], np.float64)
    assert P[2, 3] > 0.0                                  # view z = 0 (the camera) maps to depth 6 / 46 > 0
    r = _restatements_agree(spec)
    assert (r.flags == 2).sum() > 100


def test_orthographic_single_voxel_covers_exactly_the_predicted_pixel():
    """The orthographic counterpart of test_single_voxel_lands_where_the_camera_conventions_say: one voxel per pixel,
    a camera on the +x axis looking down -x with +y up (screen right is -z world, screen up is +y).  Where the voxel
    lands follows from those conventions and the extent alone, and at one voxel per pixel it covers exactly one pixel."""
    size, frame = 33, 32
    for off in [(0, 5, 0), (0, 0, 5), (0, -7, 3), (6, 4, -9)]:
        spec = testing.single_voxel_spec(off, size=size, frame=frame)
        c = size // 2
        spec.projection, spec.ortho_size = "orthographic", (float(frame), float(frame))
        # the view's centre sits on a voxel corner: pixel centres fall on voxel centres (0.5 + integer offsets)
        spec.cam_position, spec.cam_target = (c + 80.0, c + 0.5, c - 0.5), (float(c), c + 0.5, c - 0.5)
        r = lmip.render_spec(spec)
        rows, cols = np.nonzero(r.flags == 2)
        # column: screen x = -z world; pixel i's centre is at z = (c - 0.5) - (i + 0.5 - 16) = c + 15 - i
        # row: screen y = +y world; pixel j's centre is at y = (c + 0.5) + (16 - j - 0.5) = c + 16 - j
        want_col, want_row = 15 - off[2], 16 - off[1]
        assert rows.tolist() == [want_row] and cols.tolist() == [want_col], (off, rows, cols)
        assert r.label[want_row, want_col] == 7


# ---- signed and non-finite voxels (tests/special_scenes.py; the rules are in include/svr.h at svr_material) ----------
def _rel(a, b):
    """The class rule's error (tests/helpers.py) divided by max(1, |b|): the file's absolute 2e-6 for every value up
    to 1, relative above it.  The special scenes shade +-3e38 to values near 1e36, where one ulp (1e29) of libm's powf
    is far more than 2e-6 and an absolute bound cannot hold between two correct restatements."""
    from helpers import class_error

    return class_error(a, b) / np.maximum(1.0, np.abs(np.nan_to_num(b)))


@pytest.mark.parametrize("mode", ["lmip+20", "lmip-30", "lmip0", "lmip+inf", "mip", "wavg"])
@pytest.mark.parametrize("view", ["outside", "inside", "+x", "+y", "+z"])
def test_restatements_agree_on_signed_and_non_finite_voxels(view, mode):
    import special_scenes as S

    shading = list(S.SHADING)[(list(S.MARCH).index(mode) + S.VIEWS.index(view)) % len(S.SHADING)]
    spec = S.march_spec(view, mode, shading)
    a = lmip.render_spec(spec, nthreads=2, pick_id=77)
    b = lmip_numpy.render_spec(spec, pick_id=77)
    for plane in ("flags", "label", "steps", "pick"):
        np.testing.assert_array_equal(getattr(a, plane), b[plane], err_msg=plane)
    assert float(_rel(a.rgba, b["rgba"]).max()) <= 2e-6
    assert float(_rel(a.depth, b["depth"]).max()) <= 2e-6
    assert (~np.isfinite(a.rgba)).any(-1).sum() > 100               # the comparison met NaN and infinite colours


def test_mip_with_nan_voxels_follows_the_header_in_both_restatements():
    """A 32^3, 3-LOD, 48 x 40 scene with 5 % of the voxels NaN: a NaN sample neither starts nor raises the maximum
    (MIP is LMIP with threshold -inf: NaN >= -inf is false).  Before the numpy restatement said so it let a ray's first
    sample start the maximum even when NaN, and the two differed on 34 labels of 1,650 fragments."""
    rng = np.random.default_rng(5)
    pairs = []
    for l in range(3):
        n = 32 >> l
        d = rng.normal(0.0, 40.0, (n, n, n)).astype(np.float32)
        d[rng.random((n, n, n)) < 0.05] = np.nan
        pairs.append((d, rng.integers(0, 2**32, (n, n, n), dtype=np.uint64).astype(np.uint32)))
    spec = testing.synthetic_spec(32, 48, 40, pairs=pairs, chunk_shapes=[(8, 8, 8), (4, 4, 4), (2, 2, 2)],
                                  ring_shapes=[(2, 2, 2), (4, 4, 4), (8, 8, 8)])
    spec.material.update(render_mode="mip", clim=(-100.0, 100.0))
    a = lmip.render_spec(spec, nthreads=2)
    b = lmip_numpy.render_spec(spec)
    assert (b["census"]["first_nan"] & (b["flags"] == 2)).sum() >= 30         # rays whose first sample is NaN, and that still hit
    for plane in ("flags", "label", "steps"):
        np.testing.assert_array_equal(getattr(a, plane), b[plane], err_msg=plane)
    assert float(_rel(a.rgba, b["rgba"]).max()) <= 2e-6 and not np.isnan(b["census"]["sample"]).any()


@pytest.mark.parametrize("view", ["+x", "+y", "+z"])
def test_axis_views_of_the_special_scene_show_their_voxel_columns(view):
    """Known answers from the columns alone (special_scenes.column_answers, lmip_walk): MIP is the first argmax of |v|
    over the non-NaN voxels, LMIP starts at the first voxel with |v| >= threshold and walks on by the fall-off rule
    restated in scalar Python, all-NaN columns are MISS; label and depth are the winner's."""
    import ortho_scenes as ortho
    import special_scenes as S

    for mode in ("mip", "lmip+20", "lmip-30"):
        spec = S.march_spec(view, mode)
        orac = lmip.oracle_volume(spec)
        thr = spec.material["lmip_threshold"]
        ka = S.column_answers(spec, orac, "mip" if mode == "mip" else "first", thr)
        J, (iu, iv) = ka["judged"], ka["columns"]
        assert J.all()
        lo, hi = S.depth_bounds(spec, np.maximum(ka["index"], 0), ka["axis"])
        for r in (lmip.render_spec(spec, vol=orac), lmip_numpy.render_spec(spec)):
            r = r if isinstance(r, dict) else vars(r)
            np.testing.assert_array_equal(r["flags"], ka["flags"])
            if mode == "mip":
                hit = ka["flags"] == 2
                np.testing.assert_array_equal(r["label"][hit], ka["label"][hit])
                assert np.all(r["depth"][hit] >= lo[hit] - 1e-6) and np.all(r["depth"][hit] <= hi[hit] + 1e-6)
                if "census" in r:
                    np.testing.assert_array_equal(r["census"]["sample"][hit].view(np.uint32), ka["value"][hit].view(np.uint32))
                continue
            for j, i in list(zip(*np.nonzero(J)))[::37]:
                col = ortho.column_of(ka["val_xyz"], ka["axis"], 1.0, iu[j, i], iv[j, i])
                win, steps = S.lmip_walk(col, thr, 0.5, 10)
                assert steps == r["steps"][j, i] and (r["flags"][j, i] == 2) == (win >= 0), (view, mode, j, i)
                if win >= 0:
                    assert r["label"][j, i] == ortho.column_of(ka["lab_xyz"], ka["axis"], 1.0, iu[j, i], iv[j, i])[win]
                    wlo, whi = S.depth_bounds(spec, np.array(win), ka["axis"])          # the depth of the winner's voxel
                    assert wlo - 1e-6 <= r["depth"][j, i] <= whi + 1e-6, (view, mode, j, i)
