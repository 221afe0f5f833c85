"""GPU: svr_iso (include/svr.h, iso-surface render mode) == the numpy restatement of tests/iso_twin.py: flags, steps,
label and pick bit for bit, rgba, depth and normal within 1e-4, no pixel left out — u8 / u16 / float32 rings, with and
without labels, 1 and 3 LODs (every count 1 .. 8: tests/test_gpu_lod_counts.py), no / "auto" / "all" micro-block copies, perspective and orthographic cameras, a rotated
and anisotropically scaled world, clipping planes ANY and ALL, several levels / refinements / lights, and a fly-through
that wraps the rings.  Empty-space skipping: skip on == skip off on every plane bit for bit on the scenes
tests/test_gpu_skip.py builds for LMIP (2^3 blobs on cell corners and faces, levels at / just above / just below the
blob value, wrapping windows, stale maxima after asynchronous reloads, all ring types), and the counters show that
stretches really were skipped.  Also: tiles and stripes, out= in place, outline / compose on an iso render, a float
ring beyond 4 GiB, every refusal with nothing launched, and the other modes' frames bit-identical around an iso render."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import class_error
from iso_twin import iso_twin, material_of, matrices_of, params_of
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import FrameRegion, IsoResult, RenderResult, _native as N, compose, outline, testing
from test_gpu_skip import _scene, _sparse_pairs
from test_gpu_slice import spec_of

pytestmark = pytest.mark.gpu
TOL = 1e-4
PLANES = ("rgba", "depth", "label", "flags", "steps", "pick", "normal")

# iso_value as a fraction of the scene's clim[1] (the rings hold unnormalised values), then the other settings
RUNS = [
    dict(level=0.45, iso_refine=4),
    dict(level=0.30, iso_refine=0, color_by_label=True, shininess_log2=0),
    dict(level=0.60, iso_refine=16, light_direction=(0.3, -0.5, 0.8), specular=0.9, shininess_log2=10, iso_color=(0.2, 0.9, 0.4)),
    dict(level=0.45, iso_refine=3, color_by_label=True, light_direction=(-1.0, 0.2, 0.1), ambient=0.0, diffuse=1.3),
]


def host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "depth", "flags")}
    out["label"] = res.label.cpu().numpy().view(np.uint32)
    if res.steps is not None:
        out["steps"] = res.steps.cpu().numpy().view(np.uint32)
    if res.pick is not None:
        out["pick"] = res.pick.cpu().numpy().view(np.uint64)
    if getattr(res, "normal", None) is not None:
        out["normal"] = res.normal.cpu().numpy()
    return out


def check(res, ref, what):
    got = host(res) if isinstance(res, RenderResult) else res
    for k in ("flags", "steps", "label", "pick"):
        if k in got:
            print(what, k, "mismatches", int((got[k] != ref[k]).sum()))
            assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))
    for k in ("rgba", "depth", "normal"):
        if k in got:
            err = class_error(got[k].astype(np.float64), ref[k])
            print(what, k, "max abs error", float(err.max(initial=0.0)))
            assert float(err.max(initial=0.0)) <= TOL, (what, k, float(err.max(initial=0.0)))


def iso_on(vol, level=0.45, **settings):
    m = vol.material
    m.render_mode = "iso"
    m.iso_value = level
    base = dict(iso_refine=4, iso_color=(0.8, 0.8, 0.8), color_by_label=False, ambient=0.2, diffuse=0.7, specular=0.3,
                shininess_log2=5, light_direction=None)
    base.update(settings)
    for k, v in base.items():
        setattr(m, k, v)


def twin(vol, cam, spec, orac, region=None, width=None, height=None):
    return iso_twin(lmip.rings_of(orac), matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material),
                    width or spec.width, height or spec.height, params_of(vol.material), region=region, pick_id=vol.id)


def vmax_of(spec):
    return float(spec.material.get("clim", (0.0, 1.0))[1])


def render_and_check(vol, cam, spec, orac, what, runs=RUNS):
    n_hit = n_miss = 0
    for run in runs:
        run = dict(run)
        iso_on(vol, run.pop("level") * vmax_of(spec), **run)
        out = vol.iso_outputs(spec.width, spec.height, count_steps=True, pick=True)
        assert vol.render(cam, spec.width, spec.height, count_steps=True, pick=True, out=out) is out
        torch.cuda.synchronize()
        ref = twin(vol, cam, spec, orac)
        check(out, ref, (what, vol.material.iso_value, run))
        n_hit += int((ref["flags"] == HIT).sum())
        n_miss += int((ref["flags"] == MISS).sum())
    return n_hit, n_miss


CASES = [
    # scene, ring storage, micro-block copy, projection, world transform, clipping  (the composite mode's grid)
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
def test_iso_matches_restatement(name, storage, twin_copy, projection, world, clip):
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
        # rotation and anisotropic scale applied after the loads: the rings keep their contents, the rays move
        q = np.array([0.1, -0.15, 0.05, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
        vol.world.set_rotation_quaternion(q)
        vol.world.scale = (1.1, 0.9, 1.05)
    orac = lmip.oracle_volume(spec)
    n_hit, n_miss = render_and_check(vol, cam, spec, orac, (name, storage, twin_copy, projection, world, clip))
    assert n_hit > 1000 and n_miss + n_hit > 0              # (over the four runs: the comparison is not vacuous)
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


# ---- empty-space skipping ---------------------------------------------------------------------------------------
def both_ways(vol, cam, w, h):
    """One render with skipping and one without, every plane and the counters on the host."""
    frames = []
    for no_skip in (False, True):
        vol.iso_no_skip = no_skip
        out = vol.iso_outputs(w, h, count_steps=True, pick=True, skip_counters=True)
        vol.render(cam, w, h, count_steps=True, pick=True, out=out)
        torch.cuda.synchronize()
        frames.append((host(out), out.skip_counters.cpu().numpy().view(np.uint32).copy()))
    vol.iso_no_skip = False
    return frames


def assert_same_planes(on, off, what):
    for k in PLANES:
        assert np.array_equal(on[k].view(np.uint8), off[k].view(np.uint8)), (what, k, int((on[k] != off[k]).sum()))


@pytest.mark.parametrize("cam", ["K1", "K2", "-x", "+y", "-z", "diag"])
@pytest.mark.parametrize("level", [200.0, 199.5, 200.5, 5.0])
def test_sparse_bright_voxels_on_cell_borders(cam, level):
    """iso_value == the blobs' value (>= must hit), just below, just above (nothing reaches it: every ray runs to its
    end through skipped space), and inside the background noise (every cell is 'occupied'): skip on == skip off ==
    the restatement."""
    spec = _scene(128, _sparse_pairs(128, 1), level, cam)
    scene = testing.build(spec)
    vol = scene.volume
    iso_on(vol, level, iso_refine=4, color_by_label=True)
    (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
    assert_same_planes(on, off, (cam, level))
    assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0]
    ref = twin(vol, scene.camera, spec, lmip.oracle_volume(spec))
    check(on, ref, ("sparse", cam, level))
    n_hit = int((ref["flags"] == HIT).sum())
    if level > 200.0:
        assert n_hit == 0 and int((ref["flags"] == MISS).sum()) > 1000 and n_on[0] == 0
    elif level == 5.0:
        assert n_hit > 1000
    vol.close()


@pytest.mark.parametrize("storage,dtype,scale", [("native", np.uint8, 1), ("float32", np.uint8, 1), ("native", np.uint16, 257)])
def test_skip_on_equals_skip_off_and_really_skips(storage, dtype, scale):
    pairs = [(d.astype(dtype) * scale, l) for d, l in _sparse_pairs(128, 2)]
    spec = _scene(128, pairs, 150.0 * scale, "K1", storage)
    spec.material.update(clim=(0.0, 255.0 * scale))
    scene = testing.build(spec)
    vol = scene.volume
    for level in (150.0 * scale, 200.0 * scale, 200.0 * scale + 0.5):
        iso_on(vol, level, iso_refine=5)
        (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
        assert_same_planes(on, off, (storage, level))
        print(storage, level, "wave-stretches marched / skipped with skipping", n_on, "without", n_off)
        assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0]
        assert n_on[1] > 1000 and n_on[1] > n_on[0]              # a sparse scene: most stretches are passed
        check(on, twin(vol, scene.camera, spec, lmip.oracle_volume(spec)), ("really skips", storage, level))
    assert (on["flags"] == HIT).sum() == 0 and (off["flags"] == MISS).sum() > 1000       # the last level is above every voxel
    vol.close()


def test_levels_that_cannot_be_skipped_on():
    """iso_value <= 0 (float rings keep max |v|: no proof below 0) and a ring without cell grids march plainly."""
    spec = _scene(128, _sparse_pairs(128, 2), 150.0, "K1", "float32")
    scene = testing.build(spec)
    vol = scene.volume
    for level in (0.0, -3.0):
        iso_on(vol, level)
        (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
        assert_same_planes(on, off, level)
        assert n_on[1] == 0 and n_on[0] == n_off[0]
        check(on, twin(vol, scene.camera, spec, lmip.oracle_volume(spec)), ("level", level))
        assert (on["flags"] == HIT).sum() > 1000            # (every ray that meets a resident sample hits there)
    vol.close()
    # extents that are no multiple of 8: no tables, nothing skipped, the restatement's frame
    spec = testing.synthetic_spec(64, 96, 64, chunk_shapes=[(4, 4, 4)] * 3, ring_shapes=[(7, 9, 5), (5, 5, 3), (3, 3, 3)])
    spec.blocked_twin = False
    scene = testing.build(spec)
    assert all(any(e & 7 for e in b.texture.shape) for b in lmip.oracle_volume(spec).wrapping_buffers)
    vol = scene.volume
    iso_on(vol, 0.45 * vmax_of(spec))
    (on, n_on), (off, n_off) = both_ways(vol, scene.camera, spec.width, spec.height)
    assert_same_planes(on, off, "no tables")
    assert n_on[1] == 0
    check(on, twin(vol, scene.camera, spec, lmip.oracle_volume(spec)), "no tables")
    assert (on["flags"] == HIT).sum() > 100
    vol.close()


def test_stale_maxima_after_window_moves_stay_conservative():
    """Windows move (ring slots are rewritten, some cells keep slots of chunks that left the ROI), blocking and
    asynchronous; after every move skip on == skip off == the restatement."""
    pairs = _sparse_pairs(128, 3, count=120)
    spec = _scene(128, pairs, 180.0, "K2")
    scene = testing.build(spec)
    vol = scene.volume
    iso_on(vol, 180.0, color_by_label=True)
    orac = lmip.oracle_volume(spec)
    eye = np.array(spec.cam_position)
    d = np.array(spec.cam_target) - eye
    d = d / np.linalg.norm(d)
    skipped = 0
    for k in range(1, 9):
        p = eye + d * 7.0 * k
        spec.cam_position, spec.cam_target = tuple(p), tuple(p + d)
        vol.center_on_position(tuple(p), asynchronous=bool(k & 1))
        vol.poll_uploads(wait=True)
        orac.center_on_position(tuple(p))
        cam = spec.camera()
        (on, n_on), (off, _) = both_ways(vol, cam, spec.width, spec.height)
        assert_same_planes(on, off, ("move", k))
        check(on, twin(vol, cam, spec, orac), ("move", k))
        skipped += int(n_on[1])
    assert skipped > 1000
    vol.close()


# ---- the frame plumbing -----------------------------------------------------------------------------------------
def test_tiles_stripes_and_out_in_place_equal_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    W, H = 97, 61
    for run in RUNS[:3]:
        run = dict(run)
        iso_on(vol, run.pop("level") * vmax_of(spec), **run)
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
        assert (full["flags"] == HIT).sum() > 500 and (full["flags"] == DISCARD).sum() > 100
        ref = twin(vol, cam, spec, lmip.oracle_volume(spec), width=W, height=H)
        check(full, ref, ("full", run))
    vol.close()


def test_outline_and_compose_accept_an_iso_render():
    spec = testing.synthetic_spec(64, 150, 90)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    iso_on(vol, 0.45 * vmax_of(spec), color_by_label=True)
    res = vol.render(cam, 150, 90)
    torch.cuda.synchronize()
    assert int((res.flags == HIT).sum()) > 1000
    for kw in (dict(width=1), dict(width=1, depth_tolerance=0.01), dict(width=2, color_by_label=True)):
        edged = outline(vol, res, **kw)
        torch.cuda.synchronize()
        assert edged.shape == (90, 150, 4) and bool((edged != res.rgba).any()), kw
    img = compose(vol, res, background=((0.2, 0.3, 0.4, 1.0), (0.2, 0.3, 0.4, 1.0)))
    torch.cuda.synchronize()
    assert img.shape == (90, 150, 4) and img.dtype == torch.uint8
    miss = (res.flags == MISS).cpu().numpy()                # a transparent miss shows the background
    if miss.any():
        bg = compose(vol, RenderResult(torch.zeros_like(res.rgba), None, None, res.flags, None),
                     background=((0.2, 0.3, 0.4, 1.0), (0.2, 0.3, 0.4, 1.0)))
        assert np.array_equal(img.cpu().numpy()[miss], bg.cpu().numpy()[miss])
    vol.close()


def test_a_float_ring_beyond_4_gib():
    """The 8.86 GB float32 ring of test_gpu_composite: a view of the window 8.7 GB into the ring equals the restatement
    on a small ring with the same window (64-bit element indices in every gather, the taps included)."""
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


def test_other_modes_are_bit_identical_around_an_iso_render():
    from sub_volume_renderer_amd import TransferFunction

    spec = testing.synthetic_spec(64, 96, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    m.transfer_function = TransferFunction.linear(color=(0.9, 0.8, 0.6), opacity=0.2)
    modes = ("lmip", "mip", "weighted_average", "composite")

    def frames():
        out = {}
        m.color_by_label = False                            # (shared by "composite" and "iso")
        for mode in modes:
            m.render_mode = mode
            out[mode] = {k: v.copy() for k, v in host(vol.render(cam, 96, 64, pick=True)).items()}
        return out

    before = frames()
    iso_on(vol, 0.45 * vmax_of(spec), color_by_label=True)
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
    out = IsoResult(torch.full((30, 40, 4), 7.0, device=dev), torch.full((30, 40), 7.0, device=dev),
                    torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.uint8, device=dev),
                    torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.int64, device=dev),
                    normal=torch.full((30, 40, 3), 7.0, device=dev), skip_counters=torch.full((2,), 7, dtype=torch.int32, device=dev))

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

    def params(**kw):
        iso_on(vol, 0.45 * vmax_of(spec))
        ip = vol._iso_params(out)
        for k, v in kw.items():
            if k in ("iso_color", "light_direction"):
                getattr(ip, k)[:] = v
            else:
                setattr(ip, k, v)
        return ip

    def call(h, cb=None, fr=None, ip=None, ob=None, null=()):
        cb, fr, ob = cb or camera(), fr or frame(), ob or outputs()
        ip = ip or params()
        return lib.svr_iso(h, None if "cam" in null else C.byref(cb), None if "frame" in null else C.byref(fr),
                           None if "params" in null else C.byref(ip), None if "out" in null else C.byref(ob), None)

    handle = vol._rings.handle                 # the context exists, no material was sent yet
    assert call(handle) == -1 and "svr_set_material has not been called" in lib.svr_last_error().decode()
    vol.prepare()
    inf, nan = float("inf"), float("nan")
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
        (dict(ip=params(iso_value=nan)), "iso_value must not be NaN"),
        (dict(ip=params(refine=-1)), "refine must be in 0 .. 16"),
        (dict(ip=params(refine=17)), "refine must be in 0 .. 16"),
        (dict(ip=params(shininess_log2=-1)), "shininess_log2 must be in 0 .. 10"),
        (dict(ip=params(shininess_log2=11)), "shininess_log2 must be in 0 .. 10"),
        (dict(ip=params(ambient=-0.1)), "must be finite and >= 0"),
        (dict(ip=params(diffuse=inf)), "must be finite and >= 0"),
        (dict(ip=params(specular=nan)), "must be finite and >= 0"),
        (dict(ip=params(iso_color=(0.5, 1.5, 0.5))), "iso_color must be in [0, 1]"),
        (dict(ip=params(iso_color=(nan, 0.5, 0.5))), "iso_color must be in [0, 1]"),
        (dict(ip=params(headlight=0, light_direction=(0.0, 0.0, 0.0))), "light_direction must be finite and of unit length"),
        (dict(ip=params(headlight=0, light_direction=(0.0, 2.0, 0.0))), "light_direction must be finite and of unit length"),
        (dict(ip=params(headlight=0, light_direction=(nan, 1.0, 0.0))), "light_direction must be finite and of unit length"),
        (dict(ip=params(headlight=0, light_direction=(inf, 0.0, 0.0))), "light_direction must be finite and of unit length"),
    ]
    for kw, msg in cases:
        h = kw.pop("h", handle)
        assert call(h, **kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    torch.cuda.synchronize()
    for name in ("rgba", "depth", "label", "flags", "steps", "pick", "normal", "skip_counters"):
        assert bool((getattr(out, name) == 7).all()), name                     # nothing was launched
    assert call(handle, ip=params(headlight=0, light_direction=(0.0, 0.6, 0.8), iso_value=inf)) == 0       # +inf: all MISS
    torch.cuda.synchronize()
    assert not bool((out.flags == HIT).any()) and bool((out.flags == MISS).any())
    assert call(handle) == 0                                                   # the control case runs
    torch.cuda.synchronize()
    assert not bool((out.flags == 7).any()) and int((out.flags == HIT).sum()) > 100
    assert set(out.flags.unique().tolist()) <= {DISCARD, MISS, HIT}
    vol.close()
