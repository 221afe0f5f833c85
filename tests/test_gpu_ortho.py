"""GPU: the march under orthographic (parallel-ray) cameras.  Every ray of an axis-aligned orthographic view has two
direction components that are exactly zero (a perspective ray never has: its pixel centre is never on the axis), its
depth is linear in distance (w = 1) and all rays of a wave share one direction; pixel centres can be made to land
exactly on voxel faces and on the proxy box's faces (the 0/0 rays of the slab test).  Two kinds of check:

- known answers from plain numpy (no oracle): for axis-aligned views at 1 and 2 pixels per voxel a pixel's MIP value
  is the maximum of its voxel column of the composite volume, and its LMIP value the first voxel at or above the
  threshold on columns built for it;
- every plane (flags, labels, RGBA, depth, pick, step counts) held to the oracle in the hard cases: exact-zero
  directions along macro-cell faces with skipping, kernel variants, ring storages with and without the micro-block
  copy, frame regions, clipping planes parallel to the rays, a camera whose parameters change between frames, and
  seeded orthographic fuzz (tools/fuzz_parity.random_spec(ortho=True))."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ortho_scenes as ortho
from oracle import lmip
from sub_volume_renderer_amd import FrameRegion, _native as N, testing

from test_gpu_skip import _sparse_pairs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity  # noqa: E402

pytestmark = pytest.mark.gpu

ALWAYS = 0x200          # svr_set_variant bit 9: every wave takes the micro-block copy / stages bricks (test_gpu_twin.py)
NO_SKIP = 0x008         # bit 3: no empty-space skipping


def _matrices(spec, cam):
    w = spec.world()
    m = {"world": w.matrix, "world_inv": w.inverse_matrix, "cam": cam.view_matrix, "cam_inv": cam.camera_matrix,
         "proj": cam.projection_matrix, "proj_inv": cam.projection_matrix_inverse}
    return {k: np.asarray(v, np.float32) for k, v in m.items()}


def hold(spec, scene=None, region=None, variant=None, ref=None, camera=None):
    """Both kernels against the oracle on every plane, the pick plane included."""
    scene = scene or testing.build(spec)
    vol = scene.volume
    if variant is not None:
        N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")
    if ref is None:
        ref = lmip.render_spec(spec, region=region, pick_id=vol.id)
    rep = testing.hold_both_to(ref, vol, camera or scene.camera, spec.width, spec.height, region=region, pick=True)
    for r in (rep["production"], rep["instrumented"]):
        assert np.array_equal(r.pick.cpu().numpy().view(np.uint64), ref.pick)
    return scene, ref, rep


def twin_batches(volume) -> int:
    tm = (C.c_uint64 * 16)()
    N.check(N.lib().svr_debug_timers(volume._rings.handle, tm, 1), "svr_debug_timers")
    return int(tm[15])


def skipped_batches(volume) -> int:
    census = (C.c_uint32 * 8)()
    N.check(N.lib().svr_debug_counters(volume._rings.handle, census, 1), "svr_debug_counters")
    return int(census[7])


def _assert_axis_aligned(spec, view):
    a, s = ortho.AXES[view]
    d = ortho.direction_column(spec)
    assert np.count_nonzero(d) == 1 and np.sign(d[a]) == s, d      # two exact zeros in the matrices the kernel gets


# ---- every view family, pixel centres on voxel centres, voxel faces and box faces -----------------------------------
def _family_base(width=64, height=64):
    from sub_volume_renderer_amd import synth

    pairs = [synth.volume(32, k, 64) for k in range(2)]
    # LOD 0's 16^3 window wraps around its ring and ends inside the view; LOD 1 covers the rest
    return ortho.base_spec(pairs, [(8, 8, 8), (4, 4, 4)], [(2, 2, 2), (4, 4, 4)], width, height,
                           centre=(13.0, 18.0, 11.0), lmip_threshold=120.0)


@pytest.mark.parametrize("view", ["+x", "-x", "+y", "-y", "+z", "-z"])
@pytest.mark.parametrize("ppv,face", [(1, False), (1, True), (2, True)], ids=["centres", "faces", "faces-2ppv"])
def test_axis_views(view, ppv, face):
    spec = ortho.axis_view(_family_base(64 * ppv, 64 * ppv), view, ppv=ppv, face=face)
    _assert_axis_aligned(spec, view)
    if face:
        near, _ = ortho.pixel_rays(spec)
        size = ortho.size_xyz(spec)
        for k in [k for k in range(3) if k != ortho.AXES[view][0]]:
            assert np.any(near[k] == -0.5) and np.any(near[k] == size[k] - 0.5)      # rays along both box faces
            assert np.count_nonzero(ortho.face_distance(near[k]) == 0.0) >= near[k].size // 2
    _, ref, rep = hold(spec)
    assert rep["n_hit"] > 100 and rep["n_discard"] > 100


@pytest.mark.parametrize("family", ["rot-x", "rot-y", "roll-z", "oblique", "inside--z", "inside-oblique"])
def test_rotated_oblique_and_inside_views(family):
    spec = _family_base(64, 32)
    spec.projection, spec.ortho_size, spec.depth_range = "orthographic", (48.0, 24.0), (1.0, 200.0)
    if family.startswith(("rot", "roll")):
        axis = "xyz".index(family[-1])
        c, s = 0.6, 0.8
        R = np.eye(3)
        i, j = [k for k in range(3) if k != axis]
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        cam = spec.camera()
        cam.world.position = tuple(np.array([15.5, 15.5, 15.5]) + 60.0 * (R @ np.array([0.0, 0.0, 1.0])))
        cam.world.rotation_matrix = R
        spec.camera = lambda cam=cam: cam
        d = ortho.direction_column(spec)
        if axis == 2:                                      # a roll about the view axis: the direction stays -z
            assert np.count_nonzero(d) == 1 and d[2] < 0, d
        else:                                              # one exact zero, two oblique components
            assert np.count_nonzero(d) == 2 and d[axis] == 0.0, d
    elif family == "oblique":
        spec.cam_position, spec.cam_target = (70.0, -35.0, 52.0), (15.5, 15.5, 15.5)
        assert np.all(ortho.direction_column(spec) != 0.0)
    else:
        eye = np.array([14.0, 17.0, 12.0])
        d = (0, 0, -1.0) if family == "inside--z" else (0.5, -0.3, 0.8)
        spec.ortho_size = (32.0, 16.0)
        spec.cam_position, spec.cam_target = tuple(eye), tuple(eye + np.array(d))
        spec.depth_range = (-6.0, 40.0)                    # near plane behind the camera
    _, _, rep = hold(spec)
    assert rep["n_hit"] > 100


# ---- known answers from plain numpy --------------------------------------------------------------------------------
def _rois(volume):
    out = []
    for l, b in enumerate(volume.wrapping_buffers):
        u = b.uniform_buffer.data
        assert np.all(u["scale_factor"] == np.float32(0.5 ** l))
        off, shp = tuple(int(v) for v in u["current_logical_offset_in_pixels"]), tuple(int(v) for v in u["current_logical_shape_in_pixels"])
        out.append(None if not all(shp) else (off, shp))
    return out


KA_CHUNKS, KA_RINGS = [(8, 8, 8), (4, 4, 4), (2, 2, 2)], [(2, 2, 2), (4, 4, 4), (8, 8, 8)]
KA_CENTRE = (13.0, 18.0, 11.0)        # LOD 0's window: a 16^3 box starting off the ring's grid (it wraps), inside the view


def _ka_pairs(rng, mode, dtype, view, thr):
    n = 32
    hi = {np.uint8: 255, np.uint16: 65535, np.float32: 1000.0}[dtype]
    labels = [rng.integers(1, 2**31, (n >> l,) * 3).astype(np.uint32) for l in range(3)]
    if mode == "mip":
        # independent values >= 1 per LOD: the composite is what decides every pixel
        vals = [rng.integers(1, int(hi) + 1, (n >> l,) * 3) for l in range(3)]
        return [(v.astype(dtype), s) for v, s in zip(vals, labels)]
    # LMIP: values constant on 4^3 blocks (every LOD holds the same function, whichever serves a voxel) and, along
    # the view's axis in ray order, below the threshold before a column's first block at or above it and never
    # increasing after it; a quarter of the columns never reach it
    a, s = ortho.AXES[view]
    nb = n // 4
    blocks = np.empty((nb, nb, nb), np.float64)                   # [ray order, u, v]
    lo, top = 1.0, float(hi)
    first = rng.integers(0, nb, (nb, nb))
    first[rng.random((nb, nb)) < 0.25] = nb
    for b in range(nb):
        below = rng.integers(int(lo), int(thr), (nb, nb)).astype(np.float64)
        at = rng.integers(int(thr), int(top) + 1, (nb, nb)).astype(np.float64)
        prev = blocks[b - 1] if b else at
        after = np.maximum(prev - rng.integers(0, int(thr) // 2 + 1, (nb, nb)), lo)
        blocks[b] = np.where(b < first, below, np.where(b == first, at, after))
    if s < 0:
        blocks = blocks[::-1]
    others = [k for k in range(3) if k != a]
    xyz = np.moveaxis(blocks, [0, 1, 2], [a, others[0], others[1]])    # [x, y, z] blocks
    fine = xyz.repeat(4, 0).repeat(4, 1).repeat(4, 2).transpose(2, 1, 0)   # numpy [z, y, x]
    return [(fine[::1 << l, ::1 << l, ::1 << l].astype(dtype), lab) for l, lab in enumerate(labels)]


def _known_answer(spec, vol, mode, thr):
    """Expected flags, value, label and depth interval per pixel (NaN / -1 where excluded), from numpy alone."""
    a, sign, (iu, iv), inside, edge = ortho.columns(spec)
    val, lab = ortho.composite(spec.pairs, _rois(vol))
    val_xyz, lab_xyz = val.transpose(2, 1, 0), lab.transpose(2, 1, 0)
    size = ortho.size_xyz(spec)
    H, W = inside.shape
    flags = np.zeros((H, W), np.uint8)
    value = np.full((H, W), np.nan)
    label = np.zeros((H, W), np.uint32)
    hit_index = np.full((H, W), -1)
    for j, i in zip(*np.nonzero(inside & ~edge)):
        col = ortho.column_of(val_xyz, a, sign, iu[j, i], iv[j, i])
        k = int(np.argmax(col)) if mode == "mip" else int(np.argmax(col >= thr))
        if mode == "lmip" and not col[k] >= thr:
            flags[j, i] = 1
            continue
        flags[j, i] = 2
        value[j, i] = col[k]
        label[j, i] = ortho.column_of(lab_xyz, a, sign, iu[j, i], iv[j, i])[k]
        hit_index[j, i] = k if sign > 0 else int(size[a]) - 1 - k           # data index along the ray's axis
    return flags, value, label, hit_index, inside & ~edge, a


def _depth_bounds(spec, hit_index, a):
    """fs_main.wgsl:61-72 writes the depth of proj * cam * world * (coord - 0.5), coord the NORMALISED hit coordinate:
    for a hit in voxel k along the axis that is the orthographic depth of a point between k / size - 0.5 and
    (k + 1) / size - 0.5 on that axis (the others do not move an axis-aligned orthographic depth)."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    pc = M["proj"] @ M["cam"] @ M["world"]
    size = ortho.size_xyz(spec)[a]

    def depth(t):
        p = np.zeros((4,) + t.shape)
        p[a], p[3] = t - 0.5, 1.0
        c = np.einsum("rc,c...->r...", pc, p)
        return c[2] / c[3]

    d0, d1 = depth(hit_index / size), depth((hit_index + 1) / size)
    return np.minimum(d0, d1), np.maximum(d0, d1)


@pytest.mark.parametrize("twin", ["auto", "all", False], ids=["twin-auto", "twin-all", "twin-off"])
@pytest.mark.parametrize("dtype,storage", [(np.uint8, "native"), (np.uint16, "native"), (np.float32, "native")],
                         ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("mode", ["mip", "lmip"])
def test_known_answers_of_axis_views(mode, dtype, storage, twin):
    rng = np.random.default_rng(7)
    hi = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1000.0}[dtype]
    thr = float(int(0.6 * hi))
    want_density = {np.uint8: "uint8", np.uint16: "uint16", np.float32: "float32"}[dtype]
    for n_view, (view, ppv) in enumerate([("+x", 1), ("-y", 2), ("-z", 1), ("+z", 2)]):
        pairs = _ka_pairs(rng, mode, dtype, view, thr)
        spec = ortho.base_spec(pairs, KA_CHUNKS, KA_RINGS, 64, 64 if ppv == 1 else 32, centre=KA_CENTRE,
                               lmip_threshold=thr, lmip_fall_off=0.5, lmip_max_samples=10, fog_density=0.0,
                               colors=[(0.0, 0.0, 1.0)], clim=(0.0, hi), render_mode=mode)
        spec.colorspace, spec.ring_storage, spec.blocked_twin = "linear", storage, twin
        ortho.axis_view(spec, view, ppv=ppv)
        _assert_axis_aligned(spec, view)
        scene = testing.build(spec)
        vol = scene.volume
        assert vol._rings.density_storage == want_density
        assert bool(vol._rings.blocked_twin[0]) == (twin is not False)
        rois = _rois(vol)
        # LOD 0's window wraps around its ring and its boundary crosses the view
        assert any(o % (r * c) for o, r, c in zip(rois[0][0], KA_RINGS[0], KA_CHUNKS[0]))
        assert rois[0][1] != (32, 32, 32) and rois[1][1] != (16, 16, 16)          # three LODs serve the view
        flags, value, label, hit_index, judged, a = _known_answer(spec, vol, mode, thr)
        assert judged.sum() >= 0.2 * judged.size and (flags[judged] == 2).sum() > 100
        if mode == "lmip":
            assert (flags[judged] == 1).sum() > 20
        lo, hi_d = _depth_bounds(spec, np.maximum(hit_index, 0), a)
        variants = [0] + ([ALWAYS] if twin is not False else [])
        for variant in variants:
            N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")
            twin_batches(vol)
            for r in testing.render_both(vol, scene.camera, spec.width, spec.height):
                f = r.flags.cpu().numpy()
                assert np.array_equal(f[judged], flags[judged]), (view, variant)
                assert np.all(f[~ortho.columns(spec)[3]] == 0)                    # off the volume: discarded
                hit = judged & (flags == 2)
                got = r.rgba.cpu().numpy()
                want = ((value[hit] - 0.0) / hi).astype(np.float32)             # grey, linear, no fog: rgb = the value
                for ch in range(3):
                    np.testing.assert_allclose(got[..., ch][hit], want, rtol=2e-6, atol=0)
                assert np.array_equal(r.label_numpy()[hit], label[hit]), (view, variant)
                dep = r.depth.cpu().numpy()[hit]
                assert np.all(dep >= lo[hit] - 1e-6) and np.all(dep <= hi_d[hit] + 1e-6)
            if variant == ALWAYS:
                assert twin_batches(vol) > 0            # the copy served gathers
        del scene, vol


# ---- oracle parity in the hard cases -------------------------------------------------------------------------------
def _sparse_spec(threshold, view, face=False, mode="lmip", **kw):
    spec = ortho.base_spec(_sparse_pairs(128, 1, count=400), [(8, 8, 16), (4, 4, 16), (2, 2, 16)], [(6, 6, 3), (12, 12, 3), (16, 16, 2)],
                           128, 128, lmip_threshold=threshold, clim=(0.0, 255.0), render_mode=mode, **kw)
    if view == "oblique":
        spec.projection, spec.ortho_size = "orthographic", (160.0, 160.0)
        spec.cam_position, spec.cam_target, spec.depth_range = (-90.0, 150.0, 200.0), (63.5, 63.5, 63.5), (1.0, 600.0)
        return spec
    ortho.axis_view(spec, view, face=face)
    # the macro cells are 8^3: with 1 px per voxel the face-aligned rays run exactly along cell faces
    return spec


@pytest.mark.parametrize("mode", ["lmip", "mip", "weighted_average"])
@pytest.mark.parametrize("view,face", [("-x", True), ("+y", False), ("-z", True), ("oblique", False)])
def test_modes_with_skip_on_and_off_along_cell_faces(mode, view, face):
    skipped = 0
    for threshold in (200.0, 199.5):
        spec = _sparse_spec(threshold, view, face, mode, weight_falloff=0.3)
        scene = None
        frames = {}
        for variant in (0, NO_SKIP):
            scene, _, rep = hold(spec, scene, variant=variant)
            n = skipped_batches(scene.volume)
            assert variant == 0 or n == 0
            skipped += n
            frames[variant] = rep["instrumented"]
        same = testing.planes_identical(frames[0], frames[NO_SKIP])
        assert all(same.values()), same
    if mode == "lmip":                                   # the threshold scenes take skips along the cell faces
        assert skipped > 0


@pytest.mark.parametrize("view", ["-x", "+y", "-z", "faces"])
def test_kernel_variants(view):
    spec = testing.synthetic_spec(128, 128, 128, threshold=0.45, chunk_shapes=[(8, 8, 16), (4, 4, 16), (2, 2, 16)],
                                  ring_shapes=[(6, 6, 3), (12, 12, 3), (16, 16, 2)])
    ortho.axis_view(spec, "-z" if view == "faces" else view, face=(view == "faces"))
    scene = testing.build(spec)
    ref = lmip.render_spec(spec, pick_id=scene.volume.id)
    assert (ref.flags == 2).sum() > 1000
    for variant in (0x000, 0x200, 0x100, 0x001, 0x250, 0x230, 0x202, 0x2200, 0x4200, 0xE202):
        hold(spec, scene, variant=variant, ref=ref)


@pytest.mark.parametrize("twin", ["all", False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("dtype,storage", [(np.uint8, "native"), (np.uint16, "native"), (np.uint8, "float32")],
                         ids=["u8rings", "u16rings", "f32rings"])
def test_ring_storages_with_and_without_the_copy(dtype, storage, twin):
    scale = 257 if dtype == np.uint16 else 1
    for view, face in (("+x", True), ("-y", False), ("oblique", False)):
        spec = _sparse_spec(100.0 * scale, view, face)
        spec.pairs = [(d.astype(dtype) * scale, l) for d, l in _sparse_pairs(128, 5, count=400, noise=120)]
        spec.material["clim"] = (0.0, 255.0 * scale)
        spec.ring_storage, spec.blocked_twin = storage, twin
        spec.centers = [((40.0, 70.0, 52.0), None)]        # a window that wraps around the ring
        scene, ref, _ = hold(spec)
        assert bool(scene.volume._rings.blocked_twin[0]) == (twin == "all")
        twin_batches(scene.volume)
        hold(spec, scene, variant=ALWAYS, ref=ref)
        assert (twin_batches(scene.volume) > 0) == (twin == "all")


def test_regions_equal_the_full_frame():
    spec = ortho.axis_view(_family_base(64, 64), "-z", face=True)
    scene, full, rep0 = hold(spec)
    whole = rep0["production"].rgba.cpu().numpy()
    for reg in (FrameRegion.tile(9, 17, 40, 30), *(FrameRegion.stripes(64, 64, r, 3, band_h=8) for r in range(3))):
        _, ref, rep = hold(spec, scene, region=reg)
        got = rep["production"].rgba.cpu().numpy()
        for row in range(reg.out_h):
            y = reg.y0 + ((row // reg.band_h) * reg.band_pitch + row % reg.band_h if reg.band_h else row)
            if y < 64:
                np.testing.assert_array_equal(ref.label[row], full.label[y, reg.x0:reg.x0 + reg.out_w])
                np.testing.assert_array_equal(got[row], whole[y, reg.x0:reg.x0 + reg.out_w])


@pytest.mark.parametrize("mode", ["ANY", "ALL"])
def test_clipping_planes_parallel_to_the_rays(mode):
    """Rays down -z; planes x = 10 and y = 20 contain the rays.  Pixel centres sit on voxel centres, so the columns at
    x = 10 lie exactly in the first plane: dot(world_pos, n) < d is false there and they stay."""
    spec = ortho.axis_view(_family_base(64, 64), "-z")
    spec.material["clipping_planes"] = [(1.0, 0.0, 0.0, 10.0), (0.0, -1.0, 0.0, -20.0)]
    spec.material["clipping_mode"] = mode
    near, _ = ortho.pixel_rays(spec)
    x, y = near[0], near[1]                                # the back face's world x, y (identity world transform)
    assert np.any(x == 10.0) and np.any(y == 20.0)
    _, ref, _ = hold(spec)
    in_volume = (x > -0.5) & (x < 31.5) & (y > -0.5) & (y < 31.5)
    behind = ((x < 10.0) | (y > 20.0)) if mode == "ANY" else ((x < 10.0) & (y > 20.0))
    assert np.all(ref.flags[behind] == 0)
    assert np.all(ref.flags[in_volume & ~behind] != 0) and (in_volume & ~behind & ((x == 10.0) | (y == 20.0))).sum() > 10


@pytest.mark.parametrize("change", ["width", "height", "zoom", "depth_range", "aspect"])
def test_camera_changes_are_never_served_from_a_stale_cache(change):
    spec = ortho.axis_view(_family_base(64, 64), "+y")
    scene = testing.build(spec)
    cam = scene.camera
    orac = lmip.oracle_volume(spec)
    for step in range(2):
        ref = lmip.render(lmip.rings_of(orac), _matrices(spec, cam), orac.volume_dimensions_shader, spec.material,
                          spec.width, spec.height, pick_id=scene.volume.id)
        hold(spec, scene, ref=ref, camera=cam)
        if step == 0:
            before = cam.projection_matrix.copy()
            if change == "width":
                cam.width = 40.0
                cam.maintain_aspect = False
            elif change == "height":
                cam.height = 96.0
            elif change == "zoom":
                cam.zoom = 1.6
            elif change == "depth_range":
                cam.depth_range = (30.0, 100.0)                 # every hit's depth moves
            else:
                cam.aspect = 0.5
            assert not np.array_equal(before, cam.projection_matrix)


@pytest.mark.parametrize("block", range(3))
def test_seeded_random_orthographic_scenes(block):
    hits = 0
    for seed in range(2000 + 20 * block, 2000 + 20 * (block + 1)):
        spec, region, variant = fuzz_parity.random_spec(seed, ortho=True)
        assert spec.projection == "orthographic"
        scene = testing.build(spec)
        N.check(N.lib().svr_set_variant(scene.volume.prepare(), variant), "svr_set_variant")
        ref = lmip.render_spec(spec, region=region, pick_id=scene.volume.id)
        try:
            rep = testing.hold_both_to(ref, scene.volume, scene.camera, scene.width, scene.height, region=region, pick=True)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} variant {hex(variant)}: {e}") from e
        for r in (rep["production"], rep["instrumented"]):
            assert np.array_equal(r.pick.cpu().numpy().view(np.uint64), ref.pick), (seed, hex(variant))
        hits += rep["n_hit"] > 0
    assert hits >= 5
