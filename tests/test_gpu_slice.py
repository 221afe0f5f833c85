"""GPU: svr_slice (include/svr.h, cross-section views) == the numpy restatement of tests/slice_twin.py: value, label,
flags and lod bit for bit, rgba within 1e-4, depth 0 — over synthetic scenes seen from outside and inside and the
multi-scale demo scene, u8 / u16 / float32 rings, a label-less volume, no / "auto" / "all" micro-block copies, three
axis-aligned and two oblique planes (one with non-orthogonal u and v), pixel sizes 0.37 / 1 / 2.5, a rotated, scaled
and translated world, gamma != 1, sRGB on and off, 1 and 3 LODs (every count 1 .. 8: tests/test_gpu_lod_counts.py).  Also: a fly-through against the source arrays,
tiles and stripes against the full frame, ordering against asynchronous uploads, a float ring beyond 4 GiB, outline /
compose on a slice, and every refusal with nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close, assert_same_bits
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, twin_of_spec
from sub_volume_renderer_amd import FrameRegion, RenderResult, SliceResult, SubVolume, _native as N, compose, outline, testing
from test_slice import expected_from_sources

pytestmark = pytest.mark.gpu
RGBA_TOL = 1e-4
PLANES = ("value", "label", "flags", "lod")


def host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "depth", "flags", "value", "lod")}
    out["label"] = res.label.cpu().numpy().view(np.uint32)
    return out


def check(res, ref, what):
    got = host(res) if isinstance(res, SliceResult) else res
    for k in PLANES:
        assert_same_bits(got[k], ref[k], (what, k))                    # value as bits, a NaN meeting any NaN
    assert_close(got["rgba"], ref["rgba"], RGBA_TOL, what)
    assert not got["depth"].any(), what


def orientations(p):
    """(name, u, v) in world units for pixel size p."""
    o1 = (np.array([0.8, 0.6, 0.0]), np.array([-0.36, 0.48, 0.8]))
    o2 = (np.array([0.7, 0.2, -0.4]), np.array([0.3, 0.9, 0.5]))        # not orthogonal, not unit length
    out = []
    for axis in ("z", "y", "x"):
        _, u, v = SubVolume.axis_slice_plane(axis, (0, 0, 0), p)
        out.append((axis, u, v))
    out += [("oblique", tuple(p * o1[0]), tuple(p * o1[1])), ("oblique_skew", tuple(p * o2[0]), tuple(p * o2[1]))]
    return out


def spec_of(name):
    if name == "demo":
        return testing.multiscale_demo_spec(96, 80, tiles=4)
    spec = testing.synthetic_spec(64, 96, 80, inside=name.startswith("k2"))
    if "u16" in name:
        spec.pairs = [(d.astype(np.uint16) * np.uint16(251), l) for d, l in spec.pairs]
        spec.material = dict(spec.material, clim=(0.0, 65535.0))
    if "nolabels" in name:
        spec.pairs = [(d, None) for d, _ in spec.pairs]
    if "1lod" in name:
        spec.pairs, spec.chunk_shapes, spec.ring_shapes = spec.pairs[:1], spec.chunk_shapes[:1], spec.ring_shapes[:1]
    return spec


CASES = [
    # scene, ring storage, micro-block copy, gamma, colorspace, world transform
    ("k1", "native", "auto", 1.0, "srgb", False),
    ("k2", "native", False, 0.7, "srgb", False),
    ("demo", "native", "all", 1.0, "srgb", False),
    ("k1", "float32", "all", 1.0, "physical", False),
    ("k1_u16", "native", "auto", 1.6, "srgb", False),
    ("k1_nolabels", "native", "all", 1.0, "srgb", False),
    ("k1_1lod", "native", "auto", 1.0, "srgb", False),
    ("k2", "native", "auto", 1.6, "srgb", True),
    ("k1_1lod", "float32", False, 0.7, "physical", True),
    ("k2_u16", "native", "all", 1.0, "physical", True),
]


@pytest.mark.parametrize("name,storage,twin,gamma,colorspace,world", CASES)
def test_slice_matches_restatement(name, storage, twin, gamma, colorspace, world):
    spec = spec_of(name)
    spec.ring_storage, spec.blocked_twin, spec.colorspace = storage, twin, colorspace
    spec.material = dict(spec.material, gamma=gamma)
    scene = testing.build(spec)
    vol = scene.volume
    expect = {"native": {"k1_u16": "uint16", "k2_u16": "uint16", "demo": "float32"}.get(name, "uint8"), "float32": "float32"}
    assert vol._rings.density_storage == expect[storage]
    assert (not vol._rings.labels) == ("nolabels" in name)
    # the demo's camera (its focus) stands outside the volume: slice through the volume next to it instead
    focus = np.array((10.0, 7.5, 7.5) if name == "demo" else spec.centers[0][0], np.float64)
    if world:
        # rotation, scale and translation applied after the loads: the rings keep their contents, the plane moves
        q = np.array([0.2, -0.3, 0.4, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
        vol.world.set_rotation_quaternion(q)
        vol.world.scale = (1.3, 0.8, 1.1)
        vol.world.position = (5.0, -7.0, 3.0)
        focus = (vol.world.matrix @ np.array([*focus, 1.0]))[:3]
    orac = lmip.oracle_volume(spec)
    n_hit = 0
    for p in (0.37, 1.0, 2.5):
        for oname, u, v in orientations(p):
            origin = tuple(focus + np.array([0.13, -0.21, 0.07]))
            res = vol.render_slice(origin, u, v, spec.width, spec.height)
            torch.cuda.synchronize()
            ref = twin_of_spec(spec, origin, u, v, spec.width, spec.height, world_inv=vol.world.inverse_matrix, vol=orac)
            check(res, ref, (name, storage, twin, p, oname))
            n_hit += int((ref["flags"] == HIT).sum())
            assert set(np.unique(ref["lod"])) <= set(range(len(spec.pairs))) | {255}
    assert n_hit > 5000


def test_fly_through_shows_the_source_voxels():
    """center_on_position moves that wrap the rings, then z- and x-normal slices on voxel centres == the sources."""
    spec = testing.synthetic_spec(64, 64, 64)
    scene = testing.build(spec)
    vol = scene.volume
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0), (30.0, 40.0, 22.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        orac = lmip.oracle_volume(spec)
        assert any(int(o) % r for b in orac.wrapping_buffers for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1]))
        z = int(position[2])
        res = vol.render_slice((31.5, 31.5, float(z)), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 64, 64)
        torch.cuda.synchronize()
        yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
        value, lod = expected_from_sources(spec, orac, (xx, yy, np.full_like(xx, z)))
        np.testing.assert_array_equal(res.value.cpu().numpy(), value)
        np.testing.assert_array_equal(res.lod.cpu().numpy(), lod)
        assert (lod == 0).sum() > 100
        x = int(position[0])
        res = vol.render_slice((float(x), 31.5, 31.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 64, 64)
        torch.cuda.synchronize()
        value, lod = expected_from_sources(spec, orac, (np.full_like(xx, x), xx, yy))
        np.testing.assert_array_equal(res.value.cpu().numpy(), value)
        np.testing.assert_array_equal(res.lod.cpu().numpy(), lod)


def test_tiles_and_stripes_assemble_to_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    scene = testing.build(spec)
    vol = scene.volume
    args = ((30.2, 33.1, 29.7), (0.9, 0.45, -0.3), (-0.15, 0.75, 1.05), 97, 61)
    full = {k: v.copy() for k, v in host(vol.render_slice(*args)).items()}
    tiled = {k: np.zeros_like(v) for k, v in full.items()}
    for x0, x1 in ((0, 40), (40, 97)):
        for y0, y1 in ((0, 33), (33, 61)):
            r = host(vol.render_slice(*args, region=FrameRegion.tile(x0, y0, x1 - x0, y1 - y0)))
            for k in tiled:
                tiled[k][y0:y1, x0:x1] = r[k]
    striped = {k: np.zeros_like(v) for k, v in full.items()}
    for rank in range(3):
        region = FrameRegion.stripes(97, 61, rank, 3, band_h=8)
        r = host(vol.render_slice(*args, region=region))
        rows = [y for y in range(61) if (y // 8) % 3 == rank]
        for k in striped:
            striped[k][rows] = r[k][:len(rows)]
        assert (r["flags"][len(rows):] == DISCARD).all()
    for k in full:
        np.testing.assert_array_equal(tiled[k].view(np.uint8), full[k].view(np.uint8))
        np.testing.assert_array_equal(striped[k].view(np.uint8), full[k].view(np.uint8))
    assert (full["flags"] == HIT).sum() > 1000 and (full["flags"] == DISCARD).sum() > 100


def test_slices_are_ordered_against_asynchronous_uploads():
    """Slices alternate between two streams while center_on_position(asynchronous=True) rewrites ring slots: a slice
    enqueued before the uploads shows the old state, and after poll_uploads(wait=True) a slice shows the new one."""
    spec = testing.synthetic_spec(96, 192, 160, inside=True, chunk_shapes=[(8, 8, 16), (4, 4, 16), (2, 2, 16)],
                                  ring_shapes=[(5, 5, 3), (8, 8, 3), (8, 8, 2)])
    scene = testing.build(spec)
    vol = scene.volume
    orac = lmip.oracle_volume(spec)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for _ in range(2):
        vol._slice_cache = {}
        outs.append(vol._slice_outputs(spec.height, spec.width))
    eye = np.array(spec.centers[0][0])
    d = np.array([0.3, 0.5, 0.81])
    pending = []

    def published_rings():
        rings = lmip.rings_of(orac)
        for ring, b in zip(rings, vol.wrapping_buffers):
            u = b.uniform_buffer.data
            ring["offset"] = tuple(int(c) for c in u["current_logical_offset_in_pixels"])
            ring["shape"] = tuple(int(c) for c in u["current_logical_shape_in_pixels"])
        return [dict(r, density=r["density"].copy(), labels=r["labels"].copy()) for r in rings]

    for k in range(1, 11):
        p = eye + d * 4.0 * k
        plane = (tuple(p), (0.0, 0.7, 0.7), (1.0, 0.0, 0.0)) if k % 2 else SubVolume.axis_slice_plane("z", tuple(p), 0.8)
        slot = k & 1
        if len(pending) == 2:
            res, rings, pl, s = pending.pop(0)
            s.synchronize()
            check(res, twin_of_spec(spec, *pl, spec.width, spec.height, vol=orac, rings=rings), ("frame", k - 2))
        with torch.cuda.stream(streams[slot]):
            res = vol.render_slice(*plane, spec.width, spec.height, out=outs[slot])
        pending.append((res, published_rings(), plane, streams[slot]))
        vol.center_on_position(tuple(p), asynchronous=True)
        orac.center_on_position(tuple(p))
    for res, rings, pl, s in pending:
        s.synchronize()
        check(res, twin_of_spec(spec, *pl, spec.width, spec.height, vol=orac, rings=rings), "tail")
    vol.poll_uploads(wait=True)
    plane = SubVolume.axis_slice_plane("x", tuple(eye + d * 40.0), 0.9)
    res = vol.render_slice(*plane, spec.width, spec.height)
    torch.cuda.synchronize()
    ref = twin_of_spec(spec, *plane, spec.width, spec.height, vol=orac, rings=published_rings())
    check(res, ref, "after poll_uploads")
    assert (ref["lod"] == 0).sum() > 500


def test_a_float_ring_beyond_4_gib():
    """The float32 ring of 1024 x 1024 x 2112 slots (8.86 GB) of test_gpu_streaming: the level-0 window lies in ring
    planes 952 .. 1023 and 0 .. 23, i.e. texels more than 8 GB into the ring.  Slices through it, read from the rows
    and from the micro-block copy, equal the restatement on a small ring with the same window."""
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
    spec.centers, small.centers = [(target, sizes)], [(target, sizes)]
    scene = testing.build(spec)
    vol = scene.volume
    assert vol._rings.density_storage == "float32" and vol._rings.blocked_twin[0]
    assert vol.wrapping_buffers[0]._current_logical_roi_in_pixels.begin[0] == 952
    orac = lmip.oracle_volume(small)
    planes = [((31.5, 31.5, 1010.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),        # ring plane 1010: 8.7 GB in
              ((31.5, 31.5, 1000.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),        # x-normal across the ring's wrap
              ((30.0, 33.0, 1001.0), (0.6, 0.3, -0.2), (-0.1, 0.5, 0.7))]
    for variant in (0, 0x100, 0x200):                 # default / rows only / the micro-block copy wherever there is one
        N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")
        for pl in planes:
            res = vol.render_slice(*pl, spec.width, spec.height)
            torch.cuda.synchronize()
            ref = twin_of_spec(small, *pl, spec.width, spec.height, vol=orac)
            check(res, ref, ("float ring beyond 4 GiB", variant, pl))
            assert (ref["lod"] == 0).sum() > 1000
    N.check(N.lib().svr_set_variant(vol.prepare(), 0), "svr_set_variant")
    vol.close()


def test_outline_and_compose_accept_a_slice():
    scene = testing.build(testing.synthetic_spec(64, 150, 90))
    vol = scene.volume
    res = vol.render_slice((31.0, 30.0, 33.0), (0.5, 0.0, 0.0), (0.0, 0.4, 0.3), 150, 90)
    as_render = RenderResult(res.rgba, res.depth, res.label, res.flags, None)
    for kw in (dict(width=1), dict(width=2, color_by_label=True, selected=[int(res.label[45, 75])], dim_unselected=0.3),
               dict(width=1, depth_tolerance=0.0)):
        a = outline(vol, res, **kw)
        b = outline(vol, as_render, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int((outline(vol, res) != res.rgba).any(-1).sum()) > 50
    img = compose(vol, res)
    torch.cuda.synchronize()
    assert img.shape == (90, 150, 4) and img.dtype == torch.uint8
    assert torch.equal(img, compose(vol, as_render))


def test_refusals_launch_nothing():
    scene = testing.build(testing.synthetic_spec(64, 40, 30))
    vol = scene.volume
    handle = vol.prepare()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = SliceResult(torch.full((30, 40, 4), 7.0, device=dev), torch.full((30, 40), 7.0, device=dev),
                      torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.uint8, device=dev),
                      None, value=torch.full((30, 40), 7.0, device=dev), lod=torch.full((30, 40), 7, dtype=torch.uint8, device=dev))
    lib = N.lib()

    def plane(**kw):
        pl = N.SlicePlane()
        pl.world_inv = N.mat_to_c(np.eye(4))
        pl.volume_dimensions[:] = (64.0, 64.0, 64.0)
        pl.origin[:], pl.u[:], pl.v[:] = (31.5, 31.5, 31.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
        for k, v in kw.items():
            getattr(pl, k)[:] = v
        return pl

    def frame(**kw):
        f = N.Frame(frame_w=40, frame_h=30, x0=0, y0=0, out_w=40, out_h=30, band_h=30, band_pitch=30)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def outputs(rgba=None, **kw):
        o = N.SliceOutputs()
        o.rgba = out.rgba.data_ptr() if rgba is None else rgba
        for name in ("depth", "label", "flags", "value", "lod"):
            setattr(o, name, getattr(out, name).data_ptr())
        return o

    def call(pl=None, fr=None, ob=None, h=handle, null=()):
        pl, fr, ob = pl or plane(), fr or frame(), ob or outputs()
        args = [h, None if "plane" in null else C.byref(pl), None if "frame" in null else C.byref(fr),
                None if "out" in null else C.byref(ob), None]
        return lib.svr_slice(*args)

    ob_null = N.SliceOutputs()
    cases = [
        (dict(h=None), "null argument"),
        (dict(null=("plane",)), "null argument"),
        (dict(null=("frame",)), "null argument"),
        (dict(null=("out",)), "null argument"),
        (dict(ob=ob_null), "null argument"),
        (dict(fr=frame(out_w=0)), "empty frame"),
        (dict(fr=frame(frame_h=0)), "empty frame"),
        (dict(fr=frame(x0=-1)), "negative tile origin"),
        (dict(pl=plane(volume_dimensions=(64.0, 0.0, 64.0))), "volume_dimensions must be >= 1"),
        (dict(pl=plane(origin=(0.0, float("nan"), 0.0))), "origin, u and v must be finite"),
        (dict(pl=plane(v=(0.0, float("inf"), 0.0))), "origin, u and v must be finite"),
        (dict(ob=outputs(rgba=out.rgba.data_ptr() + 4)), "16-byte aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    # the Python surface refuses before the C entry point
    for bad in (dict(width=0), dict(u=(0, 0, 0)), dict(v=(2.0, 0.0, 0.0)), dict(origin=(1, 2)),
                dict(region=FrameRegion.tile(30, 0, 20, 30)),
                dict(out=SliceResult(out.rgba[:, :20], None, None, None, None))):
        kw = dict(origin=(31.5, 31.5, 31.5), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), width=40, height=30, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            vol.render_slice(**kw)
    torch.cuda.synchronize()
    for name in ("rgba", "depth", "label", "flags", "value", "lod"):
        assert bool((getattr(out, name) == 7).all()), name                     # nothing was launched
    assert call() == 0                                                          # the control case runs
    torch.cuda.synchronize()
    assert not bool((out.lod == 7).any()) and int((out.flags == HIT).sum()) > 100
    assert not bool((out.depth != 0).any()) and set(out.flags.unique().tolist()) <= {DISCARD, MISS, HIT}
