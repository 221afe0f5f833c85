"""GPU: svr_composite (include/svr.h, composite render mode) == the numpy restatement of tests/composite_twin.py: flags,
steps, label and pick bit for bit, rgba and depth within 1e-4 — u8 / u16 / float32 rings, with and without labels, 1
and 3 LODs (every count 1 .. 8: tests/test_gpu_lod_counts.py), no / "auto" / "all" micro-block copies, perspective and orthographic cameras, a rotated and scaled world,
clipping planes ANY and ALL, cutoffs 1.0 / 0.99 / 0.5 with and without the label tint, and a fly-through that wraps
the rings.  Also: tiles and stripes, out= in place, outline / compose on a composite, a float ring beyond 4 GiB, the
table sent only when it changes, every refusal with nothing launched, LMIP / MIP / weighted-average frames that a
composite render leaves bit-identical, and two contexts that keep their tables, sampling and cut planes apart."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close
from composite_twin import composite_twin, material_of, matrices_of
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import FrameRegion, RenderResult, TransferFunction, _native as N, compose, outline, testing
from test_gpu_slice import spec_of

pytestmark = pytest.mark.gpu
TOL = 1e-4

FAINT = TransferFunction.linear(color=(0.9, 0.8, 0.6), opacity=0.02)
MID = TransferFunction.from_points([(0.0, (0.1, 0.2, 0.9, 0.0)), (0.3, (0.2, 0.9, 0.3, 0.08)), (0.6, (1.0, 0.6, 0.1, 0.3)),
                                    (1.0, (1.0, 1.0, 1.0, 0.6))], size=64)
OPAQUE = TransferFunction.from_points([(0.0, (0.0, 0.0, 0.0, 0.0)), (0.15, (0.3, 0.3, 0.3, 0.0)), (0.4, (1.0, 0.5, 0.2, 1.0))],
                                      size=2048)
RUNS = [(FAINT, 1.0, False), (MID, 0.99, True), (OPAQUE, 0.5, False), (MID, 0.99, False), (OPAQUE, 0.99, True)]


def host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "depth", "flags")}
    out["label"] = res.label.cpu().numpy().view(np.uint32)
    if res.steps is not None:
        out["steps"] = res.steps.cpu().numpy().view(np.uint32)
    if res.pick is not None:
        out["pick"] = res.pick.cpu().numpy().view(np.uint64)
    return out


def check(res, ref, what):
    got = host(res) if isinstance(res, RenderResult) else res
    for k in ("flags", "steps", "label", "pick"):
        if k in got:
            assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))
    for k in ("rgba", "depth"):
        assert_close(got[k].astype(np.float64), ref[k], TOL, (what, k))


def composite_on(vol, tf, cutoff, tint):
    m = vol.material
    m.render_mode, m.transfer_function, m.alpha_cutoff, m.color_by_label = "composite", tf, cutoff, tint


def twin(vol, cam, spec, orac, tf, cutoff, tint, region=None, width=None, height=None):
    return composite_twin(lmip.rings_of(orac), matrices_of(vol, cam), orac.volume_dimensions_shader,
                          material_of(spec.material), tf.device_table(vol._volume_dimensions), width or spec.width,
                          height or spec.height, cutoff, tint, region=region, pick_id=vol.id)


def render_and_check(vol, cam, spec, orac, what, runs=RUNS):
    n_hit = n_miss = 0
    for tf, cutoff, tint in runs:
        composite_on(vol, tf, cutoff, tint)
        res = vol.render(cam, spec.width, spec.height, count_steps=True, pick=True)
        torch.cuda.synchronize()
        ref = twin(vol, cam, spec, orac, tf, cutoff, tint)
        check(res, ref, (what, tf.size, cutoff, tint))
        n_hit += int((ref["flags"] == HIT).sum())
        n_miss += int((ref["flags"] == MISS).sum())
    return n_hit, n_miss


CASES = [
    # scene, ring storage, micro-block copy, projection, world transform, clipping
    ("k1", "native", "auto", "perspective", False, None),
    ("k1", "float32", False, "perspective", True, None),
    ("k1", "native", "all", "orthographic", False, "ANY"),
    ("k1_u16", "native", "auto", "orthographic", True, None),
    ("k1_nolabels", "native", "all", "perspective", False, "ALL"),
    ("k1_1lod", "float32", "auto", "perspective", False, None),
    ("k1_1lod", "native", False, "orthographic", False, None),
    ("demo", "native", "all", "perspective", False, None),
    ("demo", "native", False, "orthographic", True, None),
]


@pytest.mark.parametrize("name,storage,twin_copy,projection,world,clip", CASES)
def test_composite_matches_restatement(name, storage, twin_copy, projection, world, clip):
    spec = spec_of(name)
    spec.ring_storage, spec.blocked_twin = storage, twin_copy
    if projection == "orthographic":
        spec.projection = "orthographic"
        spec.ortho_size = (30.0, 25.0) if name == "demo" else (80.0, 80.0 * spec.height / spec.width)
    if clip:
        c = np.array(spec.centers[0][0] if name != "demo" else (10.0, 7.5, 7.5))
        spec.material = dict(spec.material, clipping_mode=clip,
                             clipping_planes=[(0.6, 0.0, 0.8, float(0.6 * c[0] + 0.8 * c[2])), (0.0, -1.0, 0.0, float(-c[1] - 6.0))])
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    expect = {"native": {"k1_u16": "uint16", "demo": "float32"}.get(name, "uint8"), "float32": "float32"}
    assert vol._rings.density_storage == expect[storage]
    assert (not vol._rings.labels) == ("nolabels" in name)
    if world:
        # rotation and scale applied after the loads: the rings keep their contents, the rays move
        q = np.array([0.1, -0.15, 0.05, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
        vol.world.set_rotation_quaternion(q)
        vol.world.scale = (1.1, 0.9, 1.05)
    orac = lmip.oracle_volume(spec)
    n_hit, n_miss = render_and_check(vol, cam, spec, orac, (name, storage, twin_copy, projection, world, clip))
    assert n_hit > 2000 and n_miss + n_hit > 0
    if clip:
        res = host(vol.render(cam, spec.width, spec.height))
        assert (res["flags"] == DISCARD).sum() > 100
    vol.close()


def test_fly_through_with_ring_wraps():
    spec = testing.synthetic_spec(64, 80, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        orac = lmip.oracle_volume(spec)
        assert any(int(o) % r for b in orac.wrapping_buffers for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1]))
        n_hit, _ = render_and_check(vol, cam, spec, orac, ("fly", position), runs=RUNS[:3])
        assert n_hit > 1000
    vol.close()


def test_tiles_stripes_and_out_in_place_equal_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    W, H = 97, 61
    for tf, cutoff, tint in RUNS[:3]:
        composite_on(vol, tf, cutoff, tint)
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
            assert (r["flags"][len(rows):] == DISCARD).all()
        dev = torch.device("cuda", torch.cuda.current_device())
        out = RenderResult(torch.full((H, W, 4), 7.0, device=dev), torch.full((H, W), 7.0, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.uint8, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.int64, device=dev))
        assert vol.render(cam, W, H, count_steps=True, pick=True, out=out) is out
        inplace = host(out)
        for k in full:
            np.testing.assert_array_equal(tiled[k].view(np.uint8), full[k].view(np.uint8), err_msg=k)
            np.testing.assert_array_equal(striped[k].view(np.uint8), full[k].view(np.uint8), err_msg=k)
            np.testing.assert_array_equal(inplace[k].view(np.uint8), full[k].view(np.uint8), err_msg=k)
        assert (full["flags"] == HIT).sum() > 1000 and (full["flags"] == DISCARD).sum() > 100
        ref = twin(vol, cam, spec, lmip.oracle_volume(spec), tf, cutoff, tint, width=W, height=H)
        check(full, ref, ("full", cutoff))
    vol.close()


def test_outline_and_compose_accept_a_composite():
    spec = testing.synthetic_spec(64, 150, 90)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    composite_on(vol, MID, 0.99, True)
    res = vol.render(cam, 150, 90)
    torch.cuda.synchronize()
    assert int((res.flags == HIT).sum()) > 1000 and bool((res.rgba[..., 3] < 1).any())
    for kw in (dict(width=1), dict(width=1, depth_tolerance=0.01), dict(width=2, color_by_label=True)):
        edged = outline(vol, res, **kw)
        torch.cuda.synchronize()
        assert edged.shape == (90, 150, 4) and bool((edged != res.rgba).any()), kw
    img = compose(vol, res, background=((0.2, 0.3, 0.4, 1.0), (0.2, 0.3, 0.4, 1.0)))
    torch.cuda.synchronize()
    assert img.shape == (90, 150, 4) and img.dtype == torch.uint8
    # a transparent miss shows the background
    miss = (res.flags == MISS).cpu().numpy()
    if miss.any():
        bg = compose(vol, RenderResult(torch.zeros_like(res.rgba), None, None, res.flags, None),
                     background=((0.2, 0.3, 0.4, 1.0), (0.2, 0.3, 0.4, 1.0)))
        assert np.array_equal(img.cpu().numpy()[miss], bg.cpu().numpy()[miss])
    vol.close()


def test_a_float_ring_beyond_4_gib():
    """The 8.86 GB float32 ring of test_gpu_slab: a view of the window 8.7 GB into the ring equals the restatement on
    a small ring with the same window."""
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
        s.cam_position, s.cam_target = (31.5 - 50.0, 31.5 + 20.0, 1000.0 - 30.0), target
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    assert vol._rings.density_storage == "float32"
    orac = lmip.oracle_volume(small)
    n_hit, _ = render_and_check(vol, cam, spec, orac, "float ring beyond 4 GiB", runs=RUNS[:3])
    assert n_hit > 3000
    vol.close()


def test_the_table_is_sent_only_when_it_or_the_volume_changes(monkeypatch):
    spec = testing.synthetic_spec(64, 48, 40)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    lib = N.lib()
    real = lib.svr_set_transfer_function
    sent = []

    def counting(handle, ptr, k):
        sent.append(int(k))
        return real(handle, ptr, k)

    monkeypatch.setattr(lib, "svr_set_transfer_function", counting)
    composite_on(vol, None, 0.99, False)
    a = host(vol.render(cam, 48, 40))
    vol.render(cam, 48, 40)
    vol.material.alpha_cutoff = 0.9                        # the material changes, the table does not
    vol.render(cam, 48, 40)
    assert sent == [256]
    vol.material.transfer_function = OPAQUE
    b = host(vol.render(cam, 48, 40))
    vol.render(cam, 48, 40)
    assert sent == [256, 2048]
    assert not np.array_equal(a["rgba"], b["rgba"])
    vol.volume_dimensions = tuple(2 * v for v in vol.volume_dimensions)
    vol.render(cam, 48, 40)
    assert sent == [256, 2048, 2048]
    torch.cuda.synchronize()
    vol.close()


def test_other_modes_are_bit_identical_around_a_composite_render():
    spec = testing.synthetic_spec(64, 96, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    modes = ("lmip", "mip", "weighted_average")

    def frames():
        out = {}
        for mode in modes:
            m.render_mode = mode
            out[mode] = {k: v.copy() for k, v in host(vol.render(cam, 96, 64, pick=True)).items()}
        return out

    before = frames()
    composite_on(vol, MID, 0.99, True)
    res = host(vol.render(cam, 96, 64, count_steps=True, pick=True))
    assert (res["flags"] == HIT).sum() > 1000
    after = frames()
    for mode in modes:
        for k in before[mode]:
            assert np.array_equal(before[mode][k].view(np.uint8), after[mode][k].view(np.uint8)), (mode, k)
        assert (before[mode]["flags"] == HIT).sum() > 500, mode
    vol.close()


def test_refusals_launch_nothing():
    spec = testing.synthetic_spec(64, 40, 30)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    lib = N.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = RenderResult(torch.full((30, 40, 4), 7.0, device=dev), torch.full((30, 40), 7.0, device=dev),
                       torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.uint8, device=dev),
                       torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.int64, device=dev))

    def outputs(rgba=None):
        o = N.Outputs()
        o.rgba = out.rgba.data_ptr() if rgba is None else rgba
        for name in ("depth", "label", "flags", "steps", "pick"):
            setattr(o, name, getattr(out, name).data_ptr())
        return o

    def frame(**kw):
        f = N.Frame(frame_w=40, frame_h=30, x0=0, y0=0, out_w=40, out_h=30, band_h=30, band_pitch=30)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def camera(**kw):
        cb = vol._camera_block_uncached(cam)
        for k, v in kw.items():
            getattr(cb, k)[:] = v
        return cb

    def call(h, cb=None, fr=None, cp=None, ob=None, null=()):
        cb, fr, ob = cb or camera(), fr or frame(), ob or outputs()
        cp = cp or N.CompositeParams(0.99, 0)
        return lib.svr_composite(h, None if "cam" in null else C.byref(cb), None if "frame" in null else C.byref(fr),
                                 None if "params" in null else C.byref(cp), None if "out" in null else C.byref(ob), None)

    handle = vol._rings.handle                 # the context exists, no material and no table were sent yet
    assert call(handle) == -1 and "svr_set_material has not been called" in lib.svr_last_error().decode()
    vol.prepare()
    assert call(handle) == -1 and "svr_set_transfer_function has not been called" in lib.svr_last_error().decode()
    good = np.ascontiguousarray(FAINT.device_table(vol._volume_dimensions))
    for table, k, msg in ((good, 1, "K must be in 2 .. 4096"), (np.zeros((4097, 4), np.float32), 4097, "K must be in"),
                          (np.where(np.arange(good.size).reshape(good.shape) == 5, np.nan, good).astype(np.float32), 256, "finite"),
                          (np.where(np.arange(good.size).reshape(good.shape) == 9, 1.5, good).astype(np.float32), 256, "finite"),
                          (np.where(np.arange(good.size).reshape(good.shape) == 2, -0.1, good).astype(np.float32), 256, "in [0, 1]")):
        assert lib.svr_set_transfer_function(handle, np.ascontiguousarray(table).ctypes.data, k) == -1, msg
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    assert lib.svr_set_transfer_function(handle, None, 256) == -1
    assert call(handle) == -1 and "svr_set_transfer_function has not been called" in lib.svr_last_error().decode()
    assert lib.svr_set_transfer_function(handle, good.ctypes.data, good.shape[0]) == 0
    cases = [
        (dict(h=None), "null argument"),
        (dict(null=("cam",)), "null argument"),
        (dict(null=("frame",)), "null argument"),
        (dict(null=("params",)), "null argument"),
        (dict(null=("out",)), "null argument"),
        (dict(ob=N.Outputs()), "null argument"),
        (dict(fr=frame(out_w=0)), "empty frame"),
        (dict(fr=frame(frame_h=0)), "empty frame"),
        (dict(fr=frame(x0=-1)), "negative tile origin"),
        (dict(cb=camera(volume_dimensions=(64.0, 0.5, 64.0))), "volume_dimensions must be >= 1"),
        (dict(cp=N.CompositeParams(0.0, 0)), "alpha_cutoff must be in (0, 1]"),
        (dict(cp=N.CompositeParams(1.0001, 0)), "alpha_cutoff must be in (0, 1]"),
        (dict(cp=N.CompositeParams(float("nan"), 1)), "alpha_cutoff must be in (0, 1]"),
        (dict(cp=N.CompositeParams(-1.0, 0)), "alpha_cutoff must be in (0, 1]"),
    ]
    for kw, msg in cases:
        h = kw.pop("h", handle)
        assert call(h, **kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    torch.cuda.synchronize()
    for name in ("rgba", "depth", "label", "flags", "steps", "pick"):
        assert bool((getattr(out, name) == 7).all()), name                     # nothing was launched
    assert call(handle) == 0                                                   # the control case runs
    torch.cuda.synchronize()
    assert not bool((out.flags == 7).any()) and int((out.flags == HIT).sum()) > 100
    assert set(out.flags.unique().tolist()) <= {DISCARD, MISS, HIT}
    vol.close()


def test_two_contexts_keep_their_mode_state_apart():
    """Table, sampling and cut planes belong to the context.  The package sends sampling and planes before every draw,
    which would hide a mix-up, so each context gets its state once (its first render) and is then drawn through the ABI
    with no setter in between, in the order A, B, A.  A context created after one was destroyed starts empty."""
    from slice_twin import twin_of_spec
    from sub_volume_renderer_amd import SubVolume
    from test_gpu_slice import check as check_slice

    W, H = 40, 30
    lib = N.lib()
    dev = torch.device("cuda", torch.cuda.current_device())

    def small_scene():                                    # 32^3 u8, one LOD
        spec = testing.synthetic_spec(32, W, H)
        spec.pairs, spec.chunk_shapes, spec.ring_shapes = spec.pairs[:1], spec.chunk_shapes[:1], spec.ring_shapes[:1]
        scene = testing.build(spec)
        assert scene.volume._rings.density_storage == "uint8" and len(scene.volume._rings.ring_shapes) == 1
        return spec, scene.volume, scene.camera

    def raw_composite(vol, cam):
        out = RenderResult(torch.full((H, W, 4), 7.0, device=dev), torch.full((H, W), 7.0, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.uint8, device=dev),
                           torch.full((H, W), 7, dtype=torch.int32, device=dev), torch.full((H, W), 7, dtype=torch.int64, device=dev))
        ob = N.Outputs()
        for name in ("rgba", "depth", "label", "flags", "steps", "pick"):
            setattr(ob, name, getattr(out, name).data_ptr())
        ob.pick_id = vol.id & 0xFFFFFFFF
        cb, fb = vol._camera_block_uncached(cam), vol.frame_block(W, H, None)
        cp = N.CompositeParams(vol.material.alpha_cutoff, 1 if vol.material.color_by_label else 0)
        rc = lib.svr_composite(vol._rings.handle, C.byref(cb), C.byref(fb), C.byref(cp), C.byref(ob), None)
        torch.cuda.synchronize()
        return rc, out

    def ref_of(spec, vol, cam):
        m, orac = vol.material, lmip.oracle_volume(spec)
        return composite_twin(lmip.rings_of(orac), matrices_of(vol, cam), orac.volume_dimensions_shader,
                              material_of(spec.material), m.transfer_function.device_table(vol._volume_dimensions), W, H,
                              m.alpha_cutoff, m.color_by_label, pick_id=vol.id, cut_planes=m.cut_planes, cut_mode=m.cut_mode,
                              linear=(m.interpolation == "linear"))

    c = (15.5, 15.5, 15.5)
    half = ([(0.8, -0.36, -0.48, 0.8 * c[0] - 0.36 * c[1] - 0.48 * c[2])], "ANY")
    wedge = ([(1.0, 0.0, 0.0, c[0]), (0.0, -1.0, 0.0, -c[1]), (0.0, 0.0, -1.0, -c[2])], "ALL")
    made = {}
    for name, tf, cutoff, tint, interpolation, (planes, mode) in (("A", MID, 0.99, True, "nearest", half),
                                                                 ("B", OPAQUE, 0.5, False, "linear", wedge)):
        spec, vol, cam = small_scene()
        composite_on(vol, tf, cutoff, tint)
        vol.material.interpolation, vol.material.cut_planes, vol.material.cut_mode = interpolation, planes, mode
        ref = ref_of(spec, vol, cam)
        check(vol.render(cam, W, H, count_steps=True, pick=True), ref, (name, "first render"))
        made[name] = (vol, cam, ref)
    assert not np.array_equal(made["A"][2]["rgba"], made["B"][2]["rgba"])
    assert all(int((ref["flags"] == HIT).sum()) > 100 for _, _, ref in made.values())
    for name in "ABA":
        vol, cam, ref = made[name]
        rc, out = raw_composite(vol, cam)
        assert rc == 0, lib.svr_last_error()
        check(out, ref, (name, "through the ABI"))
    # B goes, C comes (quite possibly at B's address): no table, nearest sampling
    made["B"][0].close()
    spec, vol, cam = small_scene()
    vol.prepare()
    rc, out = raw_composite(vol, cam)
    assert rc == -1 and "svr_composite: svr_set_transfer_function has not been called" in lib.svr_last_error().decode()
    assert bool((out.flags == 7).all())
    origin, u, v = SubVolume.axis_slice_plane("z", c, 1.0)
    res, pl, fb = vol._slice_outputs(H, W), vol._plane_struct(origin, u, v), vol.frame_block(W, H, None)
    assert lib.svr_slice(vol._rings.handle, C.byref(pl), C.byref(fb), C.byref(vol._plane_ob(res)),
                         C.c_void_p(vol._plane_stream(None))) == 0, lib.svr_last_error()
    torch.cuda.synchronize()
    near = twin_of_spec(spec, origin, u, v, W, H, linear=False)
    check_slice(res, near, "slice on the new context")
    assert int((near["flags"] == HIT).sum()) > 100
    assert not np.array_equal(near["value"], twin_of_spec(spec, origin, u, v, W, H, linear=True)["value"])
    # A is untouched by all that
    rc, out = raw_composite(*made["A"][:2])
    assert rc == 0
    check(out, made["A"][2], ("A", "after B went"))
    vol.close()
    made["A"][0].close()
