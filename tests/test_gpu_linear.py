"""GPU: interpolation="linear" (svr_set_interpolation, include/svr.h) on svr_slice, svr_slab, svr_composite and svr_iso
== the numpy restatement of tests/linear_twin.py.  Every pixel is compared: flags, label, lod, steps, pick and the
slice / slab value plane bit for bit; rgba, depth and normal within 1e-4.  Axes: u8 / u16 / float32 rings, with and
without labels, 1 and 3 LODs (every count 1 .. 8: tests/test_gpu_lod_counts.py), no / "auto" / "all" micro-block copies and slice variant bits 8 / 9, perspective and
orthographic cameras, a rotated and anisotropically scaled world, a fly-through that wraps the rings on every axis,
tiles and stripes, a slice at pixel size 0.25 and oblique ones, slab max / min / mean and N = 1, a float ring beyond
4 GiB.  Iso skipping under linear: skip on == no_skip on every plane on the scenes of tests/test_gpu_skip.py, and
stretches really are skipped.  Voxel centres: linear == nearest on the device.  Nothing existing moves: nearest frames
of the four entry points and LMIP frames are bit-identical around linear renders, and an unknown mode is refused.
Each figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import composite_twin
from helpers import class_error, same_bits_or_nan
import iso_twin
from linear_twin import composite_linear, iso_linear, slab_of_spec, slice_of_spec
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import FrameRegion, SubVolume, _native as N, testing
from test_gpu_composite import MID, OPAQUE, composite_on, host as host_render
from test_gpu_iso import assert_same_planes, host as host_iso, iso_on, vmax_of
from test_gpu_skip import _scene, _sparse_pairs
from test_gpu_slice import host as host_slice, orientations, spec_of

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's tolerance for rgba, depth and normal


def check_planes(got, ref, what, exact, close):
    for k in exact:
        bad = int((~same_bits_or_nan(got[k], ref[k])).sum())            # floats as bits, a NaN meeting any NaN
        print(what, k, "mismatching pixels", bad, "of", got[k].size)
        assert bad == 0, (what, k, bad)
    for k in close:
        a, b = got[k].astype(np.float64), ref[k].astype(np.float64)
        err = class_error(a, b)
        print(what, k, "max abs error", float(err.max(initial=0.0)))
        assert float(err.max(initial=0.0)) <= TOL, (what, k, float(err.max(initial=0.0)))


def check_slice(res, ref, what):
    got = host_slice(res) if not isinstance(res, dict) else res
    check_planes(got, ref, what, ("flags", "label", "lod", "value", "depth"), ("rgba",))


def check_render(got, ref, what):
    check_planes(got, ref, what, [k for k in ("flags", "label", "steps", "pick") if k in got],
                 [k for k in ("rgba", "depth", "normal") if k in got])


def transform(vol):
    """A rotated, anisotropically scaled world, applied after the loads: the rings keep their contents."""
    q = np.array([0.1, -0.15, 0.05, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    vol.world.set_rotation_quaternion(q)
    vol.world.scale = (1.1, 0.9, 1.05)


def build(name, storage, copy, projection="perspective"):
    spec = spec_of(name)
    spec.ring_storage, spec.blocked_twin = storage, copy
    if projection == "orthographic":
        spec.projection = "orthographic"
        spec.ortho_size = (80.0, 80.0 * spec.height / spec.width)
    scene = testing.build(spec)
    return spec, scene.volume, scene.camera


def set_variant(vol, variant):
    N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")


# scene, ring storage, micro-block copy, projection, world transform   (the grids of the nearest suites, thinned)
CASES = [
    ("k1", "native", "auto", "perspective", False),
    ("k1", "float32", "all", "orthographic", True),
    ("k1_u16", "native", "all", "perspective", True),
    ("k1_nolabels", "native", False, "orthographic", False),
    ("k1_1lod", "float32", "auto", "perspective", False),
    ("k1_1lod", "native", "all", "orthographic", True),
]


# ---- slices and slabs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,storage,copy,projection,world", CASES)
def test_linear_slices_and_slabs_match_the_restatement(name, storage, copy, projection, world):
    spec, vol, _ = build(name, storage, copy)
    focus = np.array(spec.centers[0][0], np.float64)
    if world:
        transform(vol)
        vol.world.position = (5.0, -7.0, 3.0)
        focus = (vol.world.matrix @ np.array([*focus, 1.0]))[:3]
    orac = lmip.oracle_volume(spec)
    winv = vol.world.inverse_matrix
    origin = tuple(focus + np.array([0.13, -0.21, 0.07]))
    n_hit = n_differs = 0
    planes = {}
    for variant in (0, 0x100, 0x200):                     # per LOD the cheaper layout / rows only / the copy wherever kept
        set_variant(vol, variant)
        for p in (0.25, 1.0):
            for oname, u, v in orientations(p):
                if variant and oname not in ("z", "oblique"):
                    continue
                res = vol.render_slice(origin, u, v, spec.width, spec.height, interpolation="linear")
                torch.cuda.synchronize()
                got = host_slice(res)
                if variant == 0:
                    ref = slice_of_spec(spec, origin, u, v, spec.width, spec.height, world_inv=winv, vol=orac)
                    planes[(p, oname)] = ref
                    near = host_slice(vol.render_slice(origin, u, v, spec.width, spec.height))
                    n_differs += int((near["value"] != got["value"]).sum())
                    n_hit += int((ref["flags"] == HIT).sum())
                check_slice(got, planes[(p, oname)], ("slice", name, storage, copy, variant, p, oname))
        # slabs: every mode, N = 1 .. 9, along a skew step
        u, v = orientations(0.7)[3][1:]
        w = (0.11, -0.23, 0.41)
        for samples, mode in ((1, "max"), (5, "max"), (9, "min"), (6, "mean")):
            res = vol.render_slab(origin, u, v, w, samples, spec.width, spec.height, mode=mode, interpolation="linear")
            torch.cuda.synchronize()
            got = host_slice(res)
            key = ("slab", samples, mode)
            if variant == 0:
                planes[key] = slab_of_spec(spec, origin, u, v, w, samples, mode, spec.width, spec.height, world_inv=winv, vol=orac)
            ref = planes[key]
            check_planes(got, ref, ("slab", name, storage, copy, variant, samples, mode), ("flags", "label", "lod", "value"),
                         ("rgba", "depth"))
            if samples == 1:                              # N = 1, max == the linear slice on every plane, on the device
                one = host_slice(vol.render_slice(origin, u, v, spec.width, spec.height, interpolation="linear"))
                for k in one:
                    assert np.array_equal(one[k].view(np.uint8), got[k].view(np.uint8)), ("N = 1", k)
    set_variant(vol, 0)
    print(name, "hit pixels", n_hit, "pixels whose linear value differs from the nearest", n_differs)
    assert n_hit > 5000 and n_differs > 2000
    vol.close()


def test_slab_on_a_power_of_two_volume_takes_the_general_chain():
    """64^3 is a power of two: nearest slabs run the two-op coordinate chain, linear ones the general chain."""
    spec = testing.synthetic_spec(64, 96, 80)
    scene = testing.build(spec)
    vol = scene.volume
    orac = lmip.oracle_volume(spec)
    origin, u, v, w = (30.2, 33.1, 29.7), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7), (0.2, -0.1, 0.3)
    for samples, mode in ((7, "max"), (4, "min"), (12, "mean")):
        got = host_slice(vol.render_slab(origin, u, v, w, samples, 96, 80, mode=mode, interpolation="linear"))
        ref = slab_of_spec(spec, origin, u, v, w, samples, mode, 96, 80, vol=orac)
        check_planes(got, ref, ("pow2 slab", samples, mode), ("flags", "label", "lod", "value"), ("rgba", "depth"))
    assert (ref["flags"] == HIT).sum() > 2000
    vol.close()


def test_voxel_centres_under_linear_equal_the_nearest_slice_on_the_device():
    spec = testing.synthetic_spec(64, 64, 64)
    spec.pairs, spec.chunk_shapes, spec.ring_shapes = spec.pairs[:1], spec.chunk_shapes[:1], spec.ring_shapes[:1]
    scene = testing.build(spec)
    vol = scene.volume
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0)):
        vol.center_on_position(position)
        for axis, centre in (("z", (31.5, 31.5, float(int(position[2])))), ("x", (float(int(position[0])), 31.5, 31.5))):
            plane = SubVolume.axis_slice_plane(axis, centre, 1.0)
            near = {k: a.copy() for k, a in host_slice(vol.render_slice(*plane, 64, 64)).items()}
            lin = host_slice(vol.render_slice(*plane, 64, 64, interpolation="linear"))
            assert (near["flags"] == HIT).sum() > 500
            for k in near:
                bad = int((near[k].view(np.uint8) != lin[k].view(np.uint8)).sum())
                print("centre identity", position, axis, k, "differing bytes", bad)
                assert bad == 0
    vol.close()


def test_linear_slice_tiles_and_stripes_assemble_to_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol = scene.volume
    vol.material.interpolation = "linear"               # None takes the material's value
    args = ((30.2, 33.1, 29.7), (0.9, 0.45, -0.3), (-0.15, 0.75, 1.05), 97, 61)
    full = {k: a.copy() for k, a in host_slice(vol.render_slice(*args)).items()}
    check_slice(full, slice_of_spec(spec, *args), "full frame")
    explicit = host_slice(vol.render_slice(*args, interpolation="nearest"))
    assert (explicit["value"] != full["value"]).sum() > 500      # a string overrides the material for that call
    tiled = {k: np.zeros_like(a) for k, a in full.items()}
    for x0, x1 in ((0, 40), (40, 97)):
        for y0, y1 in ((0, 33), (33, 61)):
            r = host_slice(vol.render_slice(*args, region=FrameRegion.tile(x0, y0, x1 - x0, y1 - y0)))
            for k in tiled:
                tiled[k][y0:y1, x0:x1] = r[k]
    striped = {k: np.zeros_like(a) for k, a in full.items()}
    for rank in range(3):
        r = host_slice(vol.render_slice(*args, region=FrameRegion.stripes(97, 61, rank, 3, band_h=8)))
        rows = [y for y in range(61) if (y // 8) % 3 == rank]
        for k in striped:
            striped[k][rows] = r[k][:len(rows)]
        assert (r["flags"][len(rows):] == DISCARD).all()
    for k in full:
        np.testing.assert_array_equal(tiled[k].view(np.uint8), full[k].view(np.uint8))
        np.testing.assert_array_equal(striped[k].view(np.uint8), full[k].view(np.uint8))
    vol.close()


# ---- composite and iso ------------------------------------------------------------------------------------------
def composite_ref(vol, cam, spec, orac, tf, cutoff, tint, region=None):
    return composite_linear(lmip.rings_of(orac), composite_twin.matrices_of(vol, cam), orac.volume_dimensions_shader,
                            composite_twin.material_of(spec.material), tf.device_table(vol._volume_dimensions), spec.width,
                            spec.height, cutoff, tint, region=region, pick_id=vol.id)


def iso_ref(vol, cam, spec, orac, region=None):
    return iso_linear(lmip.rings_of(orac), iso_twin.matrices_of(vol, cam), orac.volume_dimensions_shader,
                      iso_twin.material_of(spec.material), spec.width, spec.height, iso_twin.params_of(vol.material),
                      region=region, pick_id=vol.id)


ISO_RUNS = [dict(level=0.45, iso_refine=4), dict(level=0.30, iso_refine=0, color_by_label=True, shininess_log2=0),
            dict(level=0.60, iso_refine=16, light_direction=(0.3, -0.5, 0.8), specular=0.9, shininess_log2=10)]


def render_both_modes(vol, cam, spec, orac, what):
    vol.material.interpolation = "linear"
    n_hit = 0
    for tf, cutoff, tint in ((MID, 0.99, True), (OPAQUE, 0.5, False)):
        composite_on(vol, tf, cutoff, tint)
        got = host_render(vol.render(cam, spec.width, spec.height, count_steps=True, pick=True))
        torch.cuda.synchronize()
        ref = composite_ref(vol, cam, spec, orac, tf, cutoff, tint)
        check_render(got, ref, (what, "composite", tf.size, cutoff, tint))
        n_hit += int((ref["flags"] == HIT).sum())
    for run in ISO_RUNS:
        run = dict(run)
        iso_on(vol, run.pop("level") * vmax_of(spec), **run)
        out = vol.iso_outputs(spec.width, spec.height, count_steps=True, pick=True)
        vol.render(cam, spec.width, spec.height, count_steps=True, pick=True, out=out)
        torch.cuda.synchronize()
        ref = iso_ref(vol, cam, spec, orac)
        check_render(host_iso(out), ref, (what, "iso", vol.material.iso_value, run))
        n_hit += int((ref["flags"] == HIT).sum())
    return n_hit


@pytest.mark.parametrize("name,storage,copy,projection,world", CASES)
def test_linear_composite_and_iso_match_the_restatement(name, storage, copy, projection, world):
    spec, vol, cam = build(name, storage, copy, projection)
    if world:
        transform(vol)
    orac = lmip.oracle_volume(spec)
    n_hit = render_both_modes(vol, cam, spec, orac, (name, storage, copy, projection, world))
    print(name, "hit pixels over the runs", n_hit)
    assert n_hit > 2000
    vol.close()


def test_fly_through_that_wraps_every_axis():
    spec = testing.synthetic_spec(64, 80, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        orac = lmip.oracle_volume(spec)
        wraps = [int(o) % r for o, r in zip(orac.wrapping_buffers[0].uniform()["offset"], orac.wrapping_buffers[0].texture.shape[::-1])]
        print("fly-through", position, "ring wrap of the finest level", wraps)
        assert render_both_modes(vol, cam, spec, orac, ("fly", position)) > 1000
        for plane in (SubVolume.axis_slice_plane("y", position, 0.25), (position, (0.31, 0.1, 0.0), (0.0, 0.27, 0.12))):
            got = vol.render_slice(*plane, 80, 64, interpolation="linear")
            check_slice(got, slice_of_spec(spec, *plane, 80, 64, vol=orac), ("fly slice", position))
    assert all(wraps)                                      # the last window's wrap is nonzero on every axis
    vol.close()


def test_linear_render_tiles_and_stripes_equal_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    vol.material.interpolation = "linear"
    for mode in ("composite", "iso"):
        if mode == "composite":
            composite_on(vol, MID, 0.99, True)
        else:
            iso_on(vol, 0.45 * vmax_of(spec), iso_refine=4, color_by_label=True)

        def draw(region=None):
            out = vol.iso_outputs(region.out_w if region else 97, region.out_h if region else 61, count_steps=True, pick=True)
            vol.render(cam, 97, 61, count_steps=True, pick=True, out=out, region=region)
            torch.cuda.synchronize()
            return host_iso(out)

        full = draw()
        assert (full["flags"] == HIT).sum() > 500
        orac = lmip.oracle_volume(spec)
        ref = composite_ref(vol, cam, spec, orac, MID, 0.99, True) if mode == "composite" else iso_ref(vol, cam, spec, orac)
        check_render({k: a for k, a in full.items() if mode == "iso" or k != "normal"}, ref, ("full frame", mode))
        keys = [k for k in full if mode == "iso" or k != "normal"]
        for x0, x1 in ((0, 40), (40, 97)):
            for y0, y1 in ((0, 33), (33, 61)):
                r = draw(FrameRegion.tile(x0, y0, x1 - x0, y1 - y0))
                for k in keys:
                    assert np.array_equal(r[k].view(np.uint8), full[k][y0:y1, x0:x1].view(np.uint8)), (mode, "tile", k)
        for rank in range(3):
            r = draw(FrameRegion.stripes(97, 61, rank, 3, band_h=8))
            rows = [y for y in range(61) if (y // 8) % 3 == rank]
            for k in keys:
                assert np.array_equal(r[k][:len(rows)].view(np.uint8), full[k][rows].view(np.uint8)), (mode, "stripes", k)
    vol.close()


# ---- iso empty-space skipping under linear sampling ---------------------------------------------------------------
def both_ways(vol, cam, w, h):
    frames = []
    for no_skip in (False, True):
        vol.iso_no_skip = no_skip
        out = vol.iso_outputs(w, h, count_steps=True, pick=True, skip_counters=True)
        vol.render(cam, w, h, count_steps=True, pick=True, out=out)
        torch.cuda.synchronize()
        frames.append((host_iso(out), out.skip_counters.cpu().numpy().view(np.uint32).copy()))
    vol.iso_no_skip = False
    return frames


@pytest.mark.parametrize("cam", ["K1", "K2", "-x", "diag"])
def test_skipping_is_invisible_around_blobs_on_cell_borders(cam):
    """2^3 blobs of value 200 on cell corners and faces: a neighbouring cell's voxel enters the linear sample of a
    point whose own cell is dark.  Levels at, just below and just above HALF the blob value: the level a linear sample
    reaches half a voxel outside a blob's face."""
    spec = _scene(128, _sparse_pairs(128, 1), 100.0, cam)
    scene = testing.build(spec)
    vol = scene.volume
    vol.material.interpolation = "linear"
    orac = lmip.oracle_volume(spec)
    n_hit = 0
    for level in (100.0, 99.5, 100.5, 40.0):              # 40: a level the mean-pooled blobs of the coarser LODs reach too
        iso_on(vol, level, iso_refine=4, color_by_label=True)
        (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
        print(cam, level, "wave-stretches marched / skipped with skipping", n_on, "without", n_off,
              "hits", int((on["flags"] == HIT).sum()))
        assert_same_planes(on, off, (cam, level))
        assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0]
        assert n_on[1] > 0                                  # the test cannot pass by never skipping
        ref = iso_ref(vol, scene.camera, spec, orac)
        check_render(on, ref, ("sparse", cam, level))
        n_hit += int((ref["flags"] == HIT).sum())
    assert n_hit > 20                                       # (the inside camera sees blobs only through the coarser LODs)
    vol.close()


@pytest.mark.parametrize("storage,dtype,scale", [("native", np.uint8, 1), ("float32", np.uint8, 1), ("native", np.uint16, 257)])
def test_skipping_under_linear_on_every_ring_type(storage, dtype, scale):
    pairs = [(d.astype(dtype) * scale, l) for d, l in _sparse_pairs(128, 2)]
    spec = _scene(128, pairs, 150.0 * scale, "K1", storage)
    spec.material.update(clim=(0.0, 255.0 * scale))
    scene = testing.build(spec)
    vol = scene.volume
    vol.material.interpolation = "linear"
    orac = lmip.oracle_volume(spec)
    for level in (100.0 * scale, 100.0 * scale - 0.5, 100.0 * scale + 0.5, 200.0 * scale + 0.5):
        iso_on(vol, level, iso_refine=5)
        (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
        print(storage, level, "wave-stretches marched / skipped with skipping", n_on, "without", n_off)
        assert_same_planes(on, off, (storage, level))
        assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0] and n_on[1] > 0
        check_render(on, iso_ref(vol, scene.camera, spec, orac), ("ring types", storage, level))
    assert (on["flags"] == HIT).sum() == 0 and (on["flags"] == MISS).sum() > 1000     # the last level is above every voxel
    vol.close()


# ---- rings beyond 4 GiB -------------------------------------------------------------------------------------------
def test_a_float_ring_beyond_4_gib():
    """The 8.86 GB float32 ring of tests/test_gpu_slice.py (its memory budget, its window: texels more than 8 GB into the
    ring, across the ring's wrap): linear slices from the rows and from the micro-block copy, a slab, a composite and an
    iso render equal the restatement on a small ring with the same window."""
    from sub_volume_renderer_amd import synth

    pairs = []
    for k in range(2):
        d, l = synth.volume(64, k)
        pairs.append((np.tile(d, (17, 1, 1)), np.tile(l, (17, 1, 1))))
    kw = dict(threshold=0.45, chunk_shapes=[(8, 8, 16), (4, 4, 16)])
    spec = testing.synthetic_spec(64, 128, 96, pairs=pairs, ring_shapes=[(128, 128, 132), (40, 16, 4)], **kw)
    spec.ring_storage = "float32"
    small = testing.synthetic_spec(64, 128, 96, pairs=pairs, ring_shapes=[(16, 8, 4), (20, 8, 2)], **kw)
    sizes = [(96, 32, 32), (64, 32, 32)]
    target = (31.5, 31.5, 1000.0)
    for s in (spec, small):
        s.centers = [(target, sizes)]
        s.cam_position, s.cam_target = (31.5 - 50.0, 31.5 + 20.0, 1000.0 - 30.0), target       # the camera of test_gpu_iso.py's
    scene = testing.build(spec)
    vol = scene.volume
    assert vol._rings.density_storage == "float32" and vol._rings.blocked_twin[0]
    assert vol.wrapping_buffers[0]._current_logical_roi_in_pixels.begin[0] == 952
    orac = lmip.oracle_volume(small)
    planes = [((31.5, 31.5, 1010.2), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)),        # ring plane 1010: 8.7 GB in
              ((31.3, 31.5, 1000.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5)),        # x-normal across the ring's wrap
              ((30.0, 33.0, 1001.0), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7))]
    for variant in (0, 0x100, 0x200):
        set_variant(vol, variant)
        for pl in planes:
            res = vol.render_slice(*pl, spec.width, spec.height, interpolation="linear")
            torch.cuda.synchronize()
            ref = slice_of_spec(small, *pl, spec.width, spec.height, vol=orac)
            check_slice(res, ref, ("float ring beyond 4 GiB", variant, pl))
            assert (ref["lod"] == 0).sum() > 1000
        pl = planes[2]
        got = host_slice(vol.render_slab(*pl, (0.1, 0.2, 0.4), 5, spec.width, spec.height, mode="max", interpolation="linear"))
        ref = slab_of_spec(small, *pl, (0.1, 0.2, 0.4), 5, "max", spec.width, spec.height, vol=orac)
        check_planes(got, ref, ("slab beyond 4 GiB", variant), ("flags", "label", "lod", "value"), ("rgba", "depth"))
    set_variant(vol, 0)
    assert render_both_modes(vol, scene.camera, spec, orac, "float ring beyond 4 GiB") > 1000
    vol.close()


# ---- nothing existing moved ---------------------------------------------------------------------------------------
def test_nearest_frames_are_bit_identical_around_linear_renders():
    spec, vol, cam = build("k1", "native", "auto")
    w, h = spec.width, spec.height
    plane = ((30.2, 33.1, 29.7), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7))
    step = (0.2, -0.1, 0.3)
    level = 0.45 * vmax_of(spec)

    def lmip_frame():
        vol.material.render_mode = "lmip"
        vol.material.interpolation = "nearest"
        return {k: a.copy() for k, a in host_render(vol.render(cam, w, h, count_steps=True, pick=True)).items()}

    def draw(kind, interpolation):
        vol.material.interpolation = interpolation
        if kind == "slice":
            return host_slice(vol.render_slice(*plane, w, h))
        if kind == "slab":
            return host_slice(vol.render_slab(*plane, step, 5, w, h, mode="mean"))
        if kind == "composite":
            composite_on(vol, MID, 0.99, True)
            return host_render(vol.render(cam, w, h, count_steps=True, pick=True))
        iso_on(vol, level, iso_refine=4, color_by_label=True)
        out = vol.iso_outputs(w, h, count_steps=True, pick=True)
        vol.render(cam, w, h, count_steps=True, pick=True, out=out)
        return host_iso(out)

    first_lmip = lmip_frame()
    for kind in ("slice", "slab", "composite", "iso"):
        before = {k: a.copy() for k, a in draw(kind, "nearest").items()}
        linear = {k: a.copy() for k, a in draw(kind, "linear").items()}
        between = lmip_frame()
        after = draw(kind, "nearest")
        moved = sum(int((before[k].view(np.uint8) != linear[k].view(np.uint8)).sum()) for k in before)
        print(kind, "bytes a linear render changes", moved)
        assert moved > 1000
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (kind, k)
        for k in first_lmip:
            assert np.array_equal(first_lmip[k].view(np.uint8), between[k].view(np.uint8)), (kind, "lmip", k)
    # an unknown mode is refused and changes nothing: the context stays linear here, then nearest
    lib, handle = N.lib(), vol.prepare()
    vol.material.interpolation = "nearest"
    for current in ("linear", "nearest"):
        want = {k: a.copy() for k, a in host_slice(vol.render_slice(*plane, w, h, interpolation=current)).items()}
        for bad in (7, -1, 2):
            assert lib.svr_set_interpolation(handle, bad) == -1
            assert "svr_set_interpolation" in lib.svr_last_error().decode()
        pl, fb = vol._plane_struct(*[list(map(float, c)) for c in plane]), vol.frame_block(w, h, None)
        res = vol._slice_outputs(h, w)
        N.check(lib.svr_slice(handle, C.byref(pl), C.byref(fb), C.byref(vol._plane_ob(res)),
                              C.c_void_p(vol._plane_stream(None))), "svr_slice")        # straight through the C ABI
        got = host_slice(res)
        for k in want:
            assert np.array_equal(want[k].view(np.uint8), got[k].view(np.uint8)), (current, k)
    assert lib.svr_set_interpolation(None, 0) == -1
    with pytest.raises(ValueError, match="nearest texels"):
        vol.material.render_mode, vol.material.interpolation = "lmip", "linear"
        vol.render(cam, w, h)
    vol.close()
