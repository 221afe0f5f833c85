"""GPU: svr_slab (include/svr.h, thick-slab projections) == the numpy restatement of tests/slab_twin.py: value, label,
flags, lod and depth bit for bit, rgba within 1e-4 — u8 / u16 / float32 rings, with and without labels, 1 and 3 LODs (every
count 1 .. 8: tests/test_gpu_lod_counts.py),
no / "auto" / "all" micro-block copies and variant bits 0 / 8 / 9, N in {1, 2, 7, 64}, max / min / mean, three axis
slabs and an oblique one with an oblique w, a rotated, scaled and translated world, a volume whose sizes are not
powers of two.  Also: N = 1 max == svr_slice bit for bit, tiles and stripes, out= in place, outline / compose on a slab,
a float ring beyond 4 GiB, and every refusal with nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close, assert_same_bits
from oracle import lmip
from slab_twin import twin_of_spec
from slice_twin import DISCARD, HIT
from sub_volume_renderer_amd import FrameRegion, RenderResult, SliceResult, SubVolume, _native as N, compose, outline, testing
from test_gpu_slice import spec_of

pytestmark = pytest.mark.gpu
RGBA_TOL = 1e-4
PLANES = ("value", "label", "flags", "lod", "depth")
SAMPLES = (1, 2, 7, 64)
MODES = ("max", "min", "mean")


def host(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "depth", "flags", "value", "lod")}
    out["label"] = res.label.cpu().numpy().view(np.uint32)
    return out


def check(res, ref, what):
    got = host(res) if isinstance(res, SliceResult) else res
    for k in PLANES:
        assert_same_bits(got[k], ref[k], (what, k))                    # value and depth as bits, a NaN meeting any NaN
    assert_close(got["rgba"], ref["rgba"], RGBA_TOL, what)


def slabs(p, step):
    """(name, u, v, w) in world units for pixel size p and sample step `step`."""
    out = []
    for axis in ("z", "y", "x"):
        _, u, v, w = SubVolume.axis_slab_plane(axis, (0, 0, 0), p, step)
        out.append((axis, u, v, w))
    o = (np.array([0.8, 0.6, 0.0]), np.array([-0.36, 0.48, 0.8]), np.array([0.35, -0.5, 0.6]))
    out.append(("oblique", tuple(p * o[0]), tuple(p * o[1]), tuple(step * o[2])))
    return out


CASES = [
    # scene, ring storage, micro-block copy, gamma, colorspace, world transform
    ("k1", "native", "auto", 1.0, "srgb", False),
    ("k1", "float32", "all", 1.0, "physical", True),
    ("k1_u16", "native", "auto", 1.6, "srgb", False),
    ("k1_nolabels", "native", "all", 0.7, "srgb", False),
    ("k1_1lod", "native", False, 1.0, "srgb", True),
    ("demo", "native", "all", 1.0, "srgb", False),          # float rings, sizes that are not powers of two
]


@pytest.mark.parametrize("name,storage,twin,gamma,colorspace,world", CASES)
def test_slab_matches_restatement(name, storage, twin, gamma, colorspace, world):
    spec = spec_of(name)
    spec.ring_storage, spec.blocked_twin, spec.colorspace = storage, twin, colorspace
    spec.material = dict(spec.material, gamma=gamma)
    vol = testing.build(spec).volume
    expect = {"native": {"k1_u16": "uint16", "demo": "float32"}.get(name, "uint8"), "float32": "float32"}
    assert vol._rings.density_storage == expect[storage]
    assert (not vol._rings.labels) == ("nolabels" in name)
    if name == "demo":
        assert not all(float(s).is_integer() and (int(s) & (int(s) - 1)) == 0 for s in vol._volume_dimensions)
    focus = np.array((10.0, 7.5, 7.5) if name == "demo" else spec.centers[0][0], np.float64)
    if world:
        q = np.array([0.2, -0.3, 0.4, 0.0]); q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
        vol.world.set_rotation_quaternion(q)
        vol.world.scale = (1.3, 0.8, 1.1)
        vol.world.position = (5.0, -7.0, 3.0)
        focus = (vol.world.matrix @ np.array([*focus, 1.0]))[:3]
    orac = lmip.oracle_volume(spec)
    origin = tuple(focus + np.array([0.13, -0.21, 0.07]))
    n_hit = 0
    for p, step in ((1.0, 1.0), (0.9, 0.45)):
        for sname, u, v, w in slabs(p, step):
            for n in SAMPLES:
                for mode in MODES:
                    res = vol.render_slab(origin, u, v, w, n, spec.width, spec.height, mode=mode)
                    torch.cuda.synchronize()
                    ref = twin_of_spec(spec, origin, u, v, w, n, mode, spec.width, spec.height,
                                       world_inv=vol.world.inverse_matrix, vol=orac)
                    check(res, ref, (name, storage, twin, p, sname, n, mode))
                    n_hit += int((ref["flags"] == HIT).sum())
    assert n_hit > 50000


def test_routing_variants_and_one_sample_max_equals_the_slice():
    """Variant bits 0 / 8 / 9 (default routing / rows only / the micro-block copy) give the same slabs, and N = 1 max
    equals svr_slice on every plane bit for bit, under each setting and each ring type."""
    for storage in ("native", "float32"):
        spec = testing.synthetic_spec(64, 96, 80)
        spec.ring_storage, spec.blocked_twin = storage, "all"
        vol = testing.build(spec).volume
        orac = lmip.oracle_volume(spec)
        focus = spec.centers[0][0]
        handle = vol.prepare()
        for variant in (0, 0x100, 0x200):
            N.check(N.lib().svr_set_variant(handle, variant), "svr_set_variant")
            for sname, u, v, w in slabs(0.8, 1.0):
                for n, mode in ((1, "max"), (16, "max"), (64, "mean"), (7, "min")):
                    res = host(vol.render_slab(focus, u, v, w, n, spec.width, spec.height, mode=mode))
                    ref = twin_of_spec(spec, focus, u, v, w, n, mode, spec.width, spec.height, vol=orac)
                    check(res, ref, (storage, variant, sname, n, mode))
                sl = host(vol.render_slice(focus, u, v, spec.width, spec.height))
                one = host(vol.render_slab(focus, u, v, w, 1, spec.width, spec.height))
                for k in sl:
                    assert np.array_equal(sl[k].view(np.uint8), one[k].view(np.uint8)), (storage, variant, sname, k)
                assert (sl["flags"] == HIT).sum() > 500
        N.check(N.lib().svr_set_variant(handle, 0), "svr_set_variant")
        vol.close()


def test_a_slab_does_not_overwrite_the_last_slice():
    spec = testing.synthetic_spec(64, 64, 48)
    vol = testing.build(spec).volume
    o, u, v, w = SubVolume.axis_slab_plane("z", spec.centers[0][0], 1.0, 1.0)
    sl = vol.render_slice(o, u, v, 64, 48)
    before = host(sl)
    sb = vol.render_slab(o, u, v, w, 9, 64, 48)
    assert sb.rgba.data_ptr() != sl.rgba.data_ptr()
    after = host(sl)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert not np.array_equal(host(sb)["value"], before["value"])


def test_tiles_stripes_and_out_in_place_assemble_to_the_full_frame():
    spec = testing.synthetic_spec(64, 97, 61)
    vol = testing.build(spec).volume
    args = ((30.2, 33.1, 29.7), (0.9, 0.45, -0.3), (-0.15, 0.75, 1.05), (0.4, -0.3, 0.5), 7, 97, 61)
    for mode in ("max", "mean"):
        full = {k: v.copy() for k, v in host(vol.render_slab(*args, mode=mode)).items()}
        tiled = {k: np.zeros_like(v) for k, v in full.items()}
        for x0, x1 in ((0, 40), (40, 97)):
            for y0, y1 in ((0, 33), (33, 61)):
                r = host(vol.render_slab(*args, mode=mode, region=FrameRegion.tile(x0, y0, x1 - x0, y1 - y0)))
                for k in tiled:
                    tiled[k][y0:y1, x0:x1] = r[k]
        striped = {k: np.zeros_like(v) for k, v in full.items()}
        for rank in range(3):
            r = host(vol.render_slab(*args, mode=mode, region=FrameRegion.stripes(97, 61, rank, 3, band_h=8)))
            rows = [y for y in range(61) if (y // 8) % 3 == rank]
            for k in striped:
                striped[k][rows] = r[k][:len(rows)]
            assert (r["flags"][len(rows):] == DISCARD).all()
        dev = torch.device("cuda", torch.cuda.current_device())
        out = SliceResult(torch.full((61, 97, 4), 7.0, device=dev), torch.full((61, 97), 7.0, device=dev),
                          torch.full((61, 97), 7, dtype=torch.int32, device=dev),
                          torch.full((61, 97), 7, dtype=torch.uint8, device=dev), None,
                          value=torch.full((61, 97), 7.0, device=dev), lod=torch.full((61, 97), 7, dtype=torch.uint8, device=dev))
        assert vol.render_slab(*args, mode=mode, out=out) is out
        inplace = host(out)
        for k in full:
            np.testing.assert_array_equal(tiled[k].view(np.uint8), full[k].view(np.uint8))
            np.testing.assert_array_equal(striped[k].view(np.uint8), full[k].view(np.uint8))
            np.testing.assert_array_equal(inplace[k].view(np.uint8), full[k].view(np.uint8))
        assert (full["flags"] == HIT).sum() > 1000 and (full["flags"] == DISCARD).sum() > 100


def test_a_float_ring_beyond_4_gib():
    """The 8.86 GB float32 ring of test_gpu_slice: a z-slab through ring planes 8.7 GB in and an x-slab across the
    ring's wrap, from the rows and from the micro-block copy, equal the restatement on a small ring with the same
    window."""
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
    vol = testing.build(spec).volume
    assert vol._rings.density_storage == "float32" and vol._rings.blocked_twin[0]
    orac = lmip.oracle_volume(small)
    slabs_ = [(SubVolume.axis_slab_plane("z", (31.5, 31.5, 1010.0), 1.0, 1.0), 9, "max"),
              (SubVolume.axis_slab_plane("x", (31.5, 31.5, 1000.0), 1.0, 1.5), 16, "mean")]
    for variant in (0, 0x100, 0x200):
        N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")
        for sl, n, mode in slabs_:
            res = vol.render_slab(*sl, n, spec.width, spec.height, mode=mode)
            torch.cuda.synchronize()
            ref = twin_of_spec(small, *sl, n, mode, spec.width, spec.height, vol=orac)
            check(res, ref, ("float ring beyond 4 GiB", variant, n, mode))
            assert (ref["lod"] == 0).sum() > 1000
    N.check(N.lib().svr_set_variant(vol.prepare(), 0), "svr_set_variant")
    vol.close()


def test_outline_and_compose_accept_a_slab():
    vol = testing.build(testing.synthetic_spec(64, 150, 90)).volume
    res = vol.render_slab((31.0, 30.0, 33.0), (0.5, 0.0, 0.0), (0.0, 0.4, 0.3), (0.0, -0.6, 0.8), 15, 150, 90)
    torch.cuda.synchronize()
    assert bool((res.depth != 0).any())
    as_render = RenderResult(res.rgba, res.depth, res.label, res.flags, None)
    for kw in (dict(width=1), dict(width=1, depth_tolerance=0.5), dict(width=2, depth_tolerance=2.0, color_by_label=True)):
        a = outline(vol, res, **kw)
        b = outline(vol, as_render, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the depth test finds edges inside objects where the winning sample jumps in depth
    plain, tested = outline(vol, res, width=1), outline(vol, res, width=1, depth_tolerance=0.5)
    assert int((tested != plain).any(-1).sum()) > 0
    img = compose(vol, res)
    torch.cuda.synchronize()
    assert img.shape == (90, 150, 4) and img.dtype == torch.uint8
    assert torch.equal(img, compose(vol, as_render))


def test_refusals_launch_nothing():
    vol = testing.build(testing.synthetic_spec(64, 40, 30)).volume
    handle = vol.prepare()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = SliceResult(torch.full((30, 40, 4), 7.0, device=dev), torch.full((30, 40), 7.0, device=dev),
                      torch.full((30, 40), 7, dtype=torch.int32, device=dev), torch.full((30, 40), 7, dtype=torch.uint8, device=dev),
                      None, value=torch.full((30, 40), 7.0, device=dev), lod=torch.full((30, 40), 7, dtype=torch.uint8, device=dev))
    lib = N.lib()

    def params(world_inv=None, **kw):
        sp = N.SlabParams()
        sp.plane.world_inv = N.mat_to_c(np.eye(4) if world_inv is None else world_inv)
        sp.plane.volume_dimensions[:] = (64.0, 64.0, 64.0)
        sp.plane.origin[:], sp.plane.u[:], sp.plane.v[:] = (31.5, 31.5, 31.5), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
        sp.w[:], sp.w_len, sp.samples, sp.mode = (0.0, 0.0, 1.0), 1.0, 5, 0
        for k, v in kw.items():
            if k in ("origin", "u", "v", "volume_dimensions"):
                getattr(sp.plane, k)[:] = v
            elif k == "w":
                sp.w[:] = v
            else:
                setattr(sp, k, v)
        return sp

    def frame(**kw):
        f = N.Frame(frame_w=40, frame_h=30, x0=0, y0=0, out_w=40, out_h=30, band_h=30, band_pitch=30)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def outputs(rgba=None):
        o = N.SliceOutputs()
        o.rgba = out.rgba.data_ptr() if rgba is None else rgba
        for name in ("depth", "label", "flags", "value", "lod"):
            setattr(o, name, getattr(out, name).data_ptr())
        return o

    def call(sp=None, fr=None, ob=None, h=handle, null=()):
        sp, fr, ob = sp or params(), fr or frame(), ob or outputs()
        return lib.svr_slab(h, None if "params" in null else C.byref(sp), None if "frame" in null else C.byref(fr),
                            None if "out" in null else C.byref(ob), None)

    big = np.eye(4)
    big[2, 2] = 1e30
    cases = [
        (dict(h=None), "null argument"),
        (dict(null=("params",)), "null argument"),
        (dict(null=("out",)), "null argument"),
        (dict(ob=N.SliceOutputs()), "null argument"),
        (dict(fr=frame(out_w=0)), "empty frame"),
        (dict(fr=frame(x0=-1)), "negative tile origin"),
        (dict(sp=params(volume_dimensions=(64.0, 0.0, 64.0))), "volume_dimensions must be >= 1"),
        (dict(sp=params(origin=(0.0, float("nan"), 0.0))), "origin, u and v must be finite"),
        (dict(sp=params(w=(0.0, float("inf"), 0.0))), "w must be finite"),
        (dict(sp=params(w_len=float("nan"))), "w_len must be finite and >= 0"),
        (dict(sp=params(w_len=-1.0)), "w_len must be finite and >= 0"),
        (dict(sp=params(samples=0)), "samples must be in 1 .. 4096"),
        (dict(sp=params(samples=4097)), "samples must be in 1 .. 4096"),
        (dict(sp=params(mode=3)), "unknown mode"),
        (dict(sp=params(mode=-1)), "unknown mode"),
        (dict(sp=params(world_inv=big, w=(0.0, 0.0, 1e10))), "the data-space step of w must be finite"),
        (dict(ob=outputs(rgba=out.rgba.data_ptr() + 4)), "16-byte aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    for bad in (dict(samples=0), dict(mode="sum"), dict(w=(1.0, 0.0, 0.0)), dict(w=(0, 0, 1e39)),
                dict(region=FrameRegion.tile(30, 0, 20, 30)), dict(out=SliceResult(out.rgba[:, :20], None, None, None, None))):
        kw = dict(origin=(31.5, 31.5, 31.5), u=(1.0, 0.0, 0.0), v=(0.0, 1.0, 0.0), w=(0.0, 0.0, 1.0), samples=5,
                  width=40, height=30, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            vol.render_slab(**kw)
    torch.cuda.synchronize()
    for name in ("rgba", "depth", "label", "flags", "value", "lod"):
        assert bool((getattr(out, name) == 7).all()), name                     # nothing was launched
    assert call() == 0                                                          # the control case runs
    torch.cuda.synchronize()
    assert not bool((out.lod == 7).any()) and int((out.flags == HIT).sum()) > 100
    assert set(out.flags.unique().tolist()) <= {DISCARD, 1, HIT}
