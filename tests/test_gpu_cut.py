"""GPU: svr_composite and svr_iso under svr_set_cut_planes (include/svr.h, "cut planes") == their numpy twins with the
predicate of tests/cut_twin.py, compared as tests/test_gpu_iso.py::check does: flags, steps, label and pick bit for bit,
rgba, depth and normal within 1e-4, no pixel left out.  Two cuts, both opening the side towards camera K1: H, a half-space (ANY),
and W, a wedge (ALL, the octant).  Over the iso grid (u8 / u16 / float32 rings, with and without labels, 1 and 3 LODs,
the demo, perspective and orthographic cameras, a rotated and scaled world, clipping planes as well, linear sampling),
the composite mode with and without the label tint under both samplings, and: no planes == planes set and cleared, the
march untouched by planes in the context, everything cut, skipping on == off under cuts, tiles / stripes / out=, a
fly-through that wraps the rings, outline / compose downstream, and every refusal with the state unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from composite_twin import composite_twin
from iso_twin import iso_twin, material_of, matrices_of, params_of
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import FrameRegion, RenderResult, TransferFunction, _native as N, compose, outline, testing
from test_gpu_iso import PLANES, assert_same_planes, both_ways, check, host, iso_on, vmax_of
from test_gpu_skip import _scene, _sparse_pairs
from test_gpu_slice import spec_of

pytestmark = pytest.mark.gpu
MID = TransferFunction.from_points([(0.0, (0.1, 0.2, 0.9, 0.0)), (0.3, (0.2, 0.9, 0.3, 0.08)), (0.6, (1.0, 0.6, 0.1, 0.3)),
                                    (1.0, (1.0, 1.0, 1.0, 0.6))], size=64)


def cut_of(kind, c):
    """The planes and mode of the cut ``kind`` about the world point ``c``."""
    c = [float(v) for v in c]
    if kind == "H":          # a half-space: what lies towards camera K1 of the plane through c is removed
        n = (0.8, -0.36, -0.48)
        return [n + (n[0] * c[0] + n[1] * c[1] + n[2] * c[2],)], "ANY"
    assert kind == "W"       # a wedge: the octant x < c_x, y > c_y, z > c_z (towards K1) is removed
    return [(1.0, 0.0, 0.0, c[0]), (0.0, -1.0, 0.0, -c[1]), (0.0, 0.0, -1.0, -c[2])], "ALL"


def set_cut(vol, kind, c):
    vol.material.cut_planes, vol.material.cut_mode = cut_of(kind, c)


def iso_ref(vol, cam, spec, rings, orac, **kw):
    m = vol.material
    return iso_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material),
                    kw.pop("width", spec.width), kw.pop("height", spec.height), params_of(m), pick_id=vol.id,
                    cut_planes=m.cut_planes, cut_mode=m.cut_mode, linear=(m.interpolation == "linear"), **kw)


def comp_ref(vol, cam, spec, rings, orac, tf, **kw):
    m = vol.material
    return composite_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material),
                          tf.device_table(vol._volume_dimensions), kw.pop("width", spec.width),
                          kw.pop("height", spec.height), m.alpha_cutoff, m.color_by_label, pick_id=vol.id,
                          cut_planes=m.cut_planes, cut_mode=m.cut_mode, linear=(m.interpolation == "linear"), **kw)


def iso_render(vol, cam, w, h, **kw):
    out = vol.iso_outputs(w, h, count_steps=True, pick=True, **kw)
    assert vol.render(cam, w, h, count_steps=True, pick=True, out=out) is out
    torch.cuda.synchronize()
    return out


# iso_value as a fraction of clim[1], then the other settings
ISO_RUNS = [dict(level=0.30, iso_refine=4), dict(level=0.20, iso_refine=16, color_by_label=True),
            dict(level=0.30, iso_refine=0, light_direction=(0.3, -0.5, 0.8))]

ISO_CASES = [
    # scene, ring storage, projection, world transform, interpolation, clipping planes as well
    ("k1", "native", "perspective", False, "nearest", False),
    ("k1", "float32", "orthographic", True, "nearest", False),
    ("k1_u16", "native", "perspective", False, "nearest", False),
    ("k1_nolabels", "native", "perspective", False, "nearest", True),
    ("k1_1lod", "native", "perspective", False, "linear", False),
    ("demo", "native", "perspective", False, "nearest", False),
]


@pytest.mark.parametrize("kind", ["H", "W"])
@pytest.mark.parametrize("name,storage,projection,world,interpolation,clip", ISO_CASES)
def test_iso_under_a_cut_matches_the_twin(name, storage, projection, world, interpolation, clip, kind):
    spec = spec_of(name)
    spec.ring_storage = storage
    if projection == "orthographic":
        spec.projection, spec.ortho_size = "orthographic", (80.0, 80.0 * spec.height / spec.width)
    c = spec.centers[0][0]
    if clip:
        spec.material = dict(spec.material, clipping_mode="ANY", clipping_planes=[(0.0, -1.0, 0.0, float(-c[1] - 6.0))])
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    if world:
        q = np.array([0.1, -0.15, 0.05, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
        vol.world.set_rotation_quaternion(q)
        vol.world.scale = (1.1, 0.9, 1.05)
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    vol.material.interpolation = interpolation
    set_cut(vol, kind, c)
    what = (name, storage, projection, world, interpolation, clip, kind)
    for run in ISO_RUNS:
        run = dict(run)
        level = run.pop("level")
        iso_on(vol, level * vmax_of(spec), **run)
        out = iso_render(vol, cam, spec.width, spec.height)
        ref = iso_ref(vol, cam, spec, rings, orac)
        check(out, ref, (what, level, run))
        if (name, projection, level, run["iso_refine"]) == ("k1", "perspective", 0.30, 4):
            # the comparison is not vacuous: caps, hits the cut moved, hits it left alone
            uncut = iso_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material),
                             spec.width, spec.height, params_of(vol.material), pick_id=vol.id)
            hit = ref["flags"] == HIT
            both = hit & (uncut["flags"] == HIT)
            caps, changed = int((ref["cap"] >= 0).sum()), int((hit & ~(ref["iter"] == uncut["iter"])).sum())
            unchanged = int((both & (ref["iter"] == uncut["iter"])).sum())
            print(what, "caps", caps, "changed", changed, "unchanged", unchanged)
            assert caps >= 200 and changed >= 1000 and unchanged >= 300, (caps, changed, unchanged)
    if clip:
        assert (ref["flags"] == DISCARD).sum() > 100
    vol.close()


@pytest.mark.parametrize("kind", ["H", "W"])
@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
def test_composite_under_a_cut_matches_the_twin(kind, interpolation):
    spec = spec_of("k1")
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    m = vol.material
    m.render_mode, m.transfer_function, m.alpha_cutoff, m.interpolation = "composite", MID, 0.99, interpolation
    set_cut(vol, kind, spec.centers[0][0])
    for tint in (False, True):
        m.color_by_label = tint
        res = vol.render(cam, spec.width, spec.height, count_steps=True, pick=True)
        torch.cuda.synchronize()
        ref = comp_ref(vol, cam, spec, rings, orac, MID)
        check(res, {k: ref[k] for k in ("rgba", "depth", "label", "flags", "steps", "pick")}, (kind, interpolation, tint))
    planes, m.cut_planes = m.cut_planes, ()
    uncut = comp_ref(vol, cam, spec, rings, orac, MID)
    differ = int((uncut["rgba"] != ref["rgba"]).any(-1).sum())
    print(kind, interpolation, "pixels that differ from the uncut twin", differ)
    assert differ >= 1000 and planes
    vol.close()


# ---- no cuts means no change ------------------------------------------------------------------------------------------
def test_no_planes_equals_planes_set_and_cleared_and_the_march_ignores_them():
    spec = spec_of("k1")
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    m.transfer_function, m.alpha_cutoff = MID, 0.99
    w, h = spec.width, spec.height
    march = ("lmip", "mip", "weighted_average")

    def frames(modes):
        out = {}
        for mode in modes:
            m.render_mode, m.color_by_label = mode, False
            if mode == "iso":
                iso_on(vol, 0.30 * vmax_of(spec), iso_refine=4)
                out[mode] = {k: v.copy() for k, v in host(iso_render(vol, cam, w, h)).items()}
            else:
                res = vol.render(cam, w, h, count_steps=(mode == "composite"), pick=True)
                torch.cuda.synchronize()
                out[mode] = {k: v.copy() for k, v in host(res).items()}
        return out

    before = frames(march + ("composite", "iso"))                     # no planes were ever set in this context
    lib, handle = N.lib(), vol._rings.handle
    planes, mode = cut_of("W", spec.centers[0][0])
    flat = (C.c_float * 12)(*[v for p in planes for v in p])
    assert lib.svr_set_cut_planes(handle, flat, 3, N.CUT_MODES[mode]) == 0
    during = frames(march)                                            # svr_render with planes in the context
    set_cut(vol, "H", spec.centers[0][0])
    cut = frames(("composite", "iso"))
    m.cut_planes = ()
    after = frames(march + ("composite", "iso"))                      # pushed an empty list: the context is clear again
    for mode in march:
        for k in before[mode]:
            assert np.array_equal(before[mode][k].view(np.uint8), during[mode][k].view(np.uint8)), (mode, k)
    for mode in before:
        assert (before[mode]["flags"] == HIT).sum() > 500, mode
        for k in before[mode]:
            assert np.array_equal(before[mode][k].view(np.uint8), after[mode][k].view(np.uint8)), (mode, k)
    for mode in cut:
        assert (cut[mode]["rgba"] != before[mode]["rgba"]).any(-1).sum() > 1000, mode
    vol.close()


# ---- everything cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes,mode", [([(1.0, 0.0, 0.0, 1e6)], "ANY"), ([(1.0, 0.0, 0.0, 1e6), (0.0, 1.0, 0.0, 1e6)], "ALL")])
def test_everything_cut_misses_everywhere(planes, mode):
    spec = spec_of("k1")
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    m = vol.material
    m.cut_planes, m.cut_mode = planes, mode
    iso_on(vol, 0.30 * vmax_of(spec))
    out = iso_render(vol, cam, spec.width, spec.height, skip_counters=True)
    ref = iso_ref(vol, cam, spec, rings, orac)
    check(out, ref, ("all cut", mode))
    got = host(out)
    frag = ref["flags"] != DISCARD
    assert frag.sum() > 1000 and (got["flags"][frag] == MISS).all() and not (ref["flags"] == HIT).any()
    nsteps = iso_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material), spec.width,
                      spec.height, dict(params_of(m), iso_value=float("inf")))["steps"]
    assert np.array_equal(got["steps"], nsteps) and nsteps[frag].min() >= 1
    counters = out.skip_counters.cpu().numpy().view(np.uint32)
    assert counters[0] == 0 and counters[1] > 0, counters
    m.render_mode, m.transfer_function, m.alpha_cutoff = "composite", MID, 0.99
    res = host(vol.render(cam, spec.width, spec.height, count_steps=True, pick=True))
    assert (res["flags"][frag] == MISS).all() and np.array_equal(res["steps"], nsteps)
    assert not res["rgba"].any() and not res["pick"].any()
    vol.close()


# ---- skipping, tiles, rings -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["H", "W"])
def test_skipping_on_equals_skipping_off_under_a_cut(kind):
    spec = _scene(128, _sparse_pairs(128, 2), 150.0, "K1")
    scene = testing.build(spec)
    vol = scene.volume
    set_cut(vol, kind, spec.centers[0][0])
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    for level in (150.0, 5.0):                               # the blobs alone; the background noise too (caps everywhere)
        iso_on(vol, level, iso_refine=5)
        (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
        assert_same_planes(on, off, (kind, level))
        print(kind, level, "wave-stretches marched / skipped with skipping", n_on, "without", n_off)
        # stretches whose samples are all cut are passed either way; the cell maxima pass more where the level allows
        assert n_on[0] + n_on[1] == n_off[0] + n_off[1] and n_on[1] >= n_off[1] > 0
        assert level < 100.0 or n_on[1] > n_off[1]
        check(on, iso_ref(vol, scene.camera, spec, rings, orac), ("skip", kind, level))
    assert (on["flags"] == HIT).sum() > 1000
    vol.close()


def test_tiles_stripes_and_out_in_place_under_a_cut_equal_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    W, H = 97, 61
    m = vol.material
    m.transfer_function, m.alpha_cutoff = MID, 0.99
    for mode, kind in (("iso", "W"), ("composite", "H")):
        set_cut(vol, kind, spec.centers[0][0])
        if mode == "iso":
            iso_on(vol, 0.30 * vmax_of(spec), iso_refine=4, color_by_label=True)
        else:
            m.render_mode, m.color_by_label = mode, False
        full = {k: v.copy() for k, v in host(vol.render(cam, W, H, count_steps=True, pick=True)).items()}
        tiled = {k: np.zeros_like(v) for k, v in full.items()}
        for x0, x1 in ((0, 40), (40, 97)):
            for y0, y1 in ((0, 33), (33, 61)):
                r = host(vol.render(cam, W, H, count_steps=True, pick=True, region=FrameRegion.tile(x0, y0, x1 - x0, y1 - y0)))
                for k in tiled:
                    tiled[k][y0:y1, x0:x1] = r[k]
        striped = {k: np.zeros_like(v) for k, v in full.items()}
        for rank in range(3):
            r = host(vol.render(cam, W, H, count_steps=True, pick=True, region=FrameRegion.stripes(W, H, rank, 3, band_h=8)))
            rows = [y for y in range(H) if (y // 8) % 3 == rank]
            for k in striped:
                striped[k][rows] = r[k][:len(rows)]
        dev = torch.device("cuda", torch.cuda.current_device())
        out = RenderResult(torch.full((H, W, 4), 7.0, device=dev), torch.full((H, W), 7.0, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.uint8, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.int64, device=dev))
        assert vol.render(cam, W, H, count_steps=True, pick=True, out=out) is out
        inplace = host(out)
        for k in full:
            np.testing.assert_array_equal(tiled[k].view(np.uint8), full[k].view(np.uint8), err_msg=f"{mode} {k}")
            np.testing.assert_array_equal(striped[k].view(np.uint8), full[k].view(np.uint8), err_msg=f"{mode} {k}")
            np.testing.assert_array_equal(inplace[k].view(np.uint8), full[k].view(np.uint8), err_msg=f"{mode} {k}")
        assert (full["flags"] == HIT).sum() > 500
        orac = lmip.oracle_volume(spec)
        ref = (iso_ref(vol, cam, spec, lmip.rings_of(orac), orac, width=W, height=H) if mode == "iso" else
               comp_ref(vol, cam, spec, lmip.rings_of(orac), orac, MID, width=W, height=H))
        check(full, {k: ref[k] for k in full}, ("full", mode))
    vol.close()


def test_fly_through_with_ring_wraps_under_a_half_space():
    spec = testing.synthetic_spec(64, 64, 48)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    centre = spec.centers[0][0]
    iso_on(vol, 0.30 * vmax_of(spec), iso_refine=4, color_by_label=True)
    set_cut(vol, "H", centre)
    wrapped = caps = 0
    for position in ((20.0, 24.0, 30.0), (28.0, 30.0, 36.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0), (40.0, 36.0, 28.0),
                     (30.0, 40.0, 24.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        orac = lmip.oracle_volume(spec)
        wrapped += any(int(o) % r for b in orac.wrapping_buffers for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1]))
        out = iso_render(vol, cam, spec.width, spec.height)
        ref = iso_ref(vol, cam, spec, lmip.rings_of(orac), orac)
        check(out, ref, ("fly", position))
        caps += int((ref["cap"] >= 0).sum())
        assert (ref["flags"] == HIT).sum() > 300
    assert wrapped >= 4 and caps > 300
    vol.close()


# ---- downstream and refusals ------------------------------------------------------------------------------------------
def test_outline_and_compose_accept_a_cut_iso_render():
    spec = testing.synthetic_spec(64, 150, 90)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    iso_on(vol, 0.30 * vmax_of(spec), color_by_label=True)
    set_cut(vol, "W", spec.centers[0][0])
    res = vol.render(cam, 150, 90)
    torch.cuda.synchronize()
    assert int((res.flags == HIT).sum()) > 1000
    edged = outline(vol, res, width=1)
    torch.cuda.synchronize()
    assert edged.shape == (90, 150, 4) and bool((edged != res.rgba).any())
    img = compose(vol, res, background=((0.2, 0.3, 0.4, 1.0), (0.2, 0.3, 0.4, 1.0)))
    torch.cuda.synchronize()
    assert img.shape == (90, 150, 4) and img.dtype == torch.uint8
    vol.close()


def test_every_refusal_of_svr_set_cut_planes_leaves_the_state_unchanged():
    spec = spec_of("k1")
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    lib = N.lib()
    iso_on(vol, 0.30 * vmax_of(spec))
    set_cut(vol, "H", spec.centers[0][0])
    w, h = spec.width, spec.height
    want = {k: v.copy() for k, v in host(iso_render(vol, cam, w, h)).items()}
    uncut_differs = False
    handle = vol._rings.handle
    inf, nan = float("inf"), float("nan")

    def planes(*rows):
        flat = [v for r in rows for v in r]
        return (C.c_float * max(len(flat), 1))(*flat)

    ok = (1.0, 0.0, 0.0, 0.0)
    cases = [
        (planes(*[ok] * 9), 9, 0, "at most"),
        (None, 1, 0, "null planes"),
        (planes(ok), 1, 2, "mode must be"),
        (planes(ok), 1, -1, "mode must be"),
        (None, 0, 7, "mode must be"),
        (planes(ok, (nan, 0.0, 1.0, 0.0)), 2, 0, "finite"),
        (planes((1.0, 0.0, 0.0, inf)), 1, 1, "finite"),
        (planes((0.0, -inf, 0.0, 0.0)), 1, 0, "finite"),
        (planes(ok, (0.0, 0.0, 0.0, 1.0)), 2, 1, "non-zero length"),
        (planes((3e38, 3e38, 0.0, 0.0)), 1, 0, "non-zero length"),
        (planes((1e-30, 0.0, 0.0, 0.0)), 1, 0, "non-zero length"),
    ]
    svr_iso = lib.svr_iso
    for ptr, count, mode, msg in cases:
        assert lib.svr_set_cut_planes(handle, ptr, count, mode) == -1, msg
        assert "svr_set_cut_planes" in lib.svr_last_error().decode() and msg in lib.svr_last_error().decode(), lib.svr_last_error()
        # the next render (the C call itself: the Python layer would push the material's planes again) equals the previous one
        out = vol.iso_outputs(w, h, count_steps=True, pick=True)
        cb, fb, ip = vol.camera_block(cam), vol.frame_block(w, h, None), vol._iso_params(out)
        ob = N.Outputs()
        ob.rgba = out.rgba.data_ptr()
        for name in ("depth", "label", "flags", "steps", "pick"):
            setattr(ob, name, getattr(out, name).data_ptr())
        ob.pick_id = vol.id & 0xFFFFFFFF
        assert svr_iso(handle, C.byref(cb), C.byref(fb), C.byref(ip), C.byref(ob), None) == 0
        torch.cuda.synchronize()
        got = host(out)
        for k in want:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (msg, k)
    assert lib.svr_set_cut_planes(None, None, 0, 0) == -1
    assert lib.svr_set_cut_planes(handle, None, 0, 1) == 0             # the control case: clearing works, the frame changes
    vol.material.cut_planes = ()
    cleared = host(iso_render(vol, cam, w, h))
    assert (cleared["rgba"] != want["rgba"]).any(-1).sum() > 1000
    vol.close()


def test_the_march_with_cut_planes_raises_and_launches_nothing():
    spec = testing.synthetic_spec(64, 40, 30)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    dev = torch.device("cuda", torch.cuda.current_device())
    out = RenderResult(torch.full((30, 40, 4), 7.0, device=dev), torch.full((30, 40), 7.0, device=dev),
                       torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.uint8, device=dev),
                       torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.int64, device=dev))
    set_cut(vol, "H", spec.centers[0][0])
    for mode in ("lmip", "mip", "weighted_average"):
        vol.material.render_mode = mode
        with pytest.raises(ValueError, match="cut planes"):
            vol.render(cam, 40, 30, out=out, pick=True)
    torch.cuda.synchronize()
    for name in ("rgba", "depth", "label", "flags", "steps", "pick"):
        assert bool((getattr(out, name) == 7).all()), name
    vol.material.cut_planes = ()
    vol.material.render_mode = "lmip"
    assert vol.render(cam, 40, 30, out=out, pick=True) is out
    torch.cuda.synchronize()
    assert int((out.flags == HIT).sum()) > 100
    vol.close()
