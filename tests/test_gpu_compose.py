"""GPU: svr_compose (include/svr.h) on synthetic planes (compose_f64.py), held exactly where it can be.

With srgb off the build (-ffp-contract=off) leaves the kernel no freedom: all four channels equal the float32
restatement (oracle/compose_oracle.py).  With srgb on only powf may differ: alpha and inout_depth stay exact, rgb equals
floor(v) of the float64 reference on every decidable value (|v - rint(v)| > 1e-3, derivation in compose_f64.py) and is
within one level on the rest.  No share of free mismatches anywhere.  Sizes from 1 x 1 to the first frame past one pass
of the grid, NULL planes in every combination, opaque / translucent / 4096-row gradient backgrounds, the depth test's
edges as bits, a 2^20-value sRGB sweep, NaN and inf, out=, empty frames, and every refusal with nothing launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import compose_f64 as F
from oracle import compose_oracle
from sub_volume_renderer_amd import RenderResult, _native as N, testing
from sub_volume_renderer_amd.compose import compose

pytestmark = pytest.mark.gpu

ONE_PASS = 256 * 32 * 256                     # pixels one pass of compose_kernel's grid covers (compose_kernels.hip)
_state = {}


def volume():
    """The context: one 32^3 u8 volume, one LOD (svr_compose only takes its device from it)."""
    if "vol" not in _state:
        spec = testing.synthetic_spec(32, 40, 30)
        spec.pairs, spec.chunk_shapes, spec.ring_shapes = spec.pairs[:1], spec.chunk_shapes[:1], spec.ring_shapes[:1]
        _state["vol"] = testing.build(spec).volume
    return _state["vol"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(p, combo, bg, srgb, out=None):
    """compose() of the planes p under one plane combination -> (uint8 [h, w, 4], zbuf after or None)."""
    kw = F.combo_args(p, combo)
    res = RenderResult(dev(p["rgba"]), None if kw["depth"] is None else dev(kw["depth"]), None,
                       None if kw["flags"] is None else dev(kw["flags"]), None)
    z = None if kw["zbuf"] is None else dev(kw["zbuf"])
    got = compose(volume(), res, background=bg, depth_buffer=z, srgb=srgb, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy(), None if z is None else z.cpu().numpy()


def hold_case(p, combo, bg, name, capsys):
    kw = F.combo_args(p, combo)
    bottom, top = bg
    for srgb in (False, True):
        got, z = run(p, combo, bg, srgb)
        want, zwant = compose_oracle.compose(p["rgba"], bg_bottom=bottom, bg_top=top, srgb=srgb, **kw)
        if zwant is not None:
            np.testing.assert_array_equal(bits(z), bits(zwant))                  # inout_depth: exact, as bits
        if not srgb:
            np.testing.assert_array_equal(got, want)                             # nothing may differ
            continue
        np.testing.assert_array_equal(got[..., 3], want[..., 3])                 # alpha never sees powf
        v, _ = F.reference(p["rgba"], bg_bottom=bottom, bg_top=top, srgb=True, **kw)
        und, off = F.hold(got[..., :3], v[..., :3], (name, combo[0]))
        with capsys.disabled():
            print(f"\ncompose {name} {combo[0]}: {v[..., :3].size} rgb values, {und} undecidable, {off} of them one level off")


_CASES = [(fam, combo) for fam in F.FAMILIES for combo in F.COMBOS]


@pytest.mark.parametrize("family,combo", _CASES, ids=[f"{f[0]}-{c[0]}" for f, c in _CASES])
def test_compose_equals_its_references(family, combo, capsys):
    name, seed, h, w, bg = family
    assert h * w < ONE_PASS
    hold_case(F.planes(seed, h, w), combo, bg, name, capsys)


@pytest.mark.parametrize("combo", F.COMBOS, ids=[c[0] for c in F.COMBOS])
def test_compose_past_one_pass_of_the_grid(combo, capsys):
    """2048 x 1025: the smallest frame of whole 2048-pixel rows past one pass, so the last 2048 pixels are reached only
    by the grid-stride step, by the first 8 blocks of the grid alone."""
    name, seed, h, w, bg = F.BIG
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "compose_kernels.hip")).read()
    assert "std::min<size_t>((n + 255) / 256, 256 * 32)" in src, "the grid cap of svr_launch_compose changed: resize this frame"
    assert ONE_PASS == 2_097_152 and ONE_PASS < h * w == ONE_PASS + 2048
    if "big" not in _state:
        _state["big"] = F.planes(seed, h, w)
    hold_case(_state["big"], combo, bg, name, capsys)


def test_depth_test_edges_as_bits():
    """depth < inout_depth in IEEE f32: equal bits, NaN on either side and -0 against +0 are not drawn and leave the
    canvas depth's bits alone; +inf on the canvas is behind everything finite."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pairs = [(0.5, 0.5, False), (nan, 0.5, False), (0.5, nan, False), (0.5, inf, True), (-0.0, 0.0, False),
             (0.0, -0.0, False), (-inf, 0.0, True), (0.3, 0.7, True), (0.7, 0.3, False), (inf, inf, False),
             (np.nextafter(np.float32(0.5), np.float32(0)), 0.5, True), (1e-45, 0.0, False), (0.0, 1e-45, True)]
    depth = np.array([[d for d, _, _ in pairs]], np.float32)
    zbuf = np.array([[z for _, z, _ in pairs]], np.float32)
    drawn = np.array([[k for _, _, k in pairs]])
    p = dict(rgba=np.ones((1, len(pairs), 4), np.float32), depth=depth, zbuf=zbuf, flags=None)
    black = ((0, 0, 0, 1), (0, 0, 0, 1))
    for combo in (F.COMBOS[1], ("flags2_ztest", True, True, True)):
        p["flags"] = np.full(depth.shape, 2, np.uint8)
        for srgb in (False, True):
            got, z = run(p, combo, black, srgb)
            assert (got[0, :, 0] == np.where(drawn[0], 255, 0)).all() and (got[..., 3] == 255).all(), got[0, :, 0]
            np.testing.assert_array_equal(bits(z), bits(np.where(drawn, depth, zbuf)))
            want, zwant = compose_oracle.compose(p["rgba"], depth=depth, zbuf=zbuf, srgb=srgb)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(bits(z), bits(zwant))
    # a quarter of a frame's pixels at depth == zbuf bit for bit: none of them drawn, none of their depths rewritten
    fam = F.FAMILIES[3]
    q = F.planes(fam[1], fam[2], fam[3])
    same = bits(q["depth"]) == bits(q["zbuf"])
    assert 0.2 < same.mean() < 0.3
    got, z = run(q, F.COMBOS[1], fam[4], False)
    background, _ = run(dict(q, flags=np.zeros_like(q["flags"])), F.COMBOS[2], fam[4], False)    # every pixel discarded
    np.testing.assert_array_equal(got[same], background[same])
    np.testing.assert_array_equal(bits(z)[same], bits(q["zbuf"])[same])
    assert (bits(z) == bits(q["depth"]))[q["depth"] < q["zbuf"]].all() and (got != background).any(-1)[~same].sum() > 1000


def _srgb_threshold_inputs():
    """The float32 values around every place the encode changes its answer: +-2 ulp of the knee and, for each of the
    255 level thresholds (the c with srgb(c) * 255 + 0.5 = k, inverted in float64), its float32 neighbours."""
    k = np.arange(1, 256, dtype=np.float64)
    y = (k - 0.5) / 255.0
    lin, a, b = float(np.float32(12.92)), float(np.float32(1.055)), float(np.float32(0.055))
    c = np.where(y <= lin * float(F.KNEE), y / lin, ((y + b) / a) ** (1.0 / float(np.float32(1) / np.float32(2.4))))
    c32 = c.astype(np.float32)
    vals = [c32]
    for centre, n in ((c32, 1), (np.array([F.KNEE], np.float32), 2)):
        lo = hi = centre
        for _ in range(n):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            vals += [lo, hi]
    vals.append(np.array([F.KNEE], np.float32))
    return np.sort(np.concatenate(vals))


def test_srgb_sweep_is_monotone_and_exact_where_decidable(capsys):
    """1024 x 1024 opaque greys over black (the blend is s * 1 + 0 * 0 = s exactly): red sweeps i / (2^20 - 1), green
    holds the values around every threshold, each repeated to fill the frame in ascending order."""
    n = 1 << 20
    sweep = (np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)
    edge = _srgb_threshold_inputs()
    assert edge.size == 255 * 3 + 5 and (np.diff(edge) >= 0).all()
    edges = np.repeat(edge, -(-n // edge.size))[:n]
    assert np.unique(edges).size == np.unique(edge).size                        # every one of them is in the frame
    rgba = np.zeros((1024, 1024, 4), np.float32)
    rgba[..., 0], rgba[..., 1], rgba[..., 3] = sweep.reshape(1024, 1024), edges.reshape(1024, 1024), 1.0
    p = dict(rgba=rgba, flags=None, depth=None, zbuf=None)
    got, _ = run(p, F.COMBOS[0], ((0, 0, 0, 1), (0, 0, 0, 1)), True)
    v, _ = F.reference(rgba)
    for ch, name in ((0, "sweep"), (1, "thresholds")):
        levels = got[..., ch].reshape(-1).astype(np.int16)
        assert (np.diff(levels) >= 0).all(), (name, np.flatnonzero(np.diff(levels) < 0)[:4])
        if ch == 0:
            assert levels[0] == 0 and levels[-1] == 255 and np.unique(levels).size == 256
        else:                                                   # the first and the last value sit on thresholds themselves
            assert levels[0] <= 1 and levels[-1] >= 254 and np.unique(levels).size >= 254
        und, off = F.hold(got[..., ch], v[..., ch], name)
        with capsys.disabled():
            print(f"\ncompose srgb {name}: {n} values, {und} undecidable, {off} of them one level off")
    assert (got[..., 2] == 0).all() and (got[..., 3] == 255).all()
    # the threshold values are undecidable by construction (that is what they are for): they must still be within a level
    assert (~F.decidable(v[..., 1])).mean() > 0.3


def test_nan_and_inf_follow_the_contract():
    """A NaN channel quantises to 0 (fmaxf returns its other operand), +inf to 255, -inf to 0; a NaN or infinite alpha
    makes inf - inf or 0 * inf of every channel, hence 0 everywhere."""
    nan, inf = np.nan, np.inf
    rgba = np.array([[[nan, 1.0, 0.0, 1.0], [1.0, nan, nan, 1.0], [inf, -inf, 1.0, 1.0], [1.0, 1.0, 1.0, nan],
                      [1.0, 1.0, 1.0, inf], [1.0, 1.0, 1.0, -inf], [nan, nan, nan, 0.0], [inf, 1.0, 0.0, 0.0],
                      [0.0, 0.0, 0.0, 0.0]]], np.float32)
    bg = ((1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0))
    hand = [[0, 255, 0, 255], [255, 0, 0, 255], [255, 0, 255, 255], [0, 0, 0, 0],
            [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 255], [0, 255, 255, 255],          # nan * 0 = inf * 0 = NaN -> 0
            [255, 255, 255, 255]]
    p = dict(rgba=rgba, flags=None, depth=None, zbuf=None)
    for srgb in (False, True):
        got, _ = run(p, F.COMBOS[0], bg, srgb)
        assert got[0].tolist() == hand, (srgb, got[0].tolist())
        want, _ = compose_oracle.compose(rgba, bg_bottom=bg[0], bg_top=bg[1], srgb=srgb)
        np.testing.assert_array_equal(got, want)
    # a NaN in the background is a NaN channel too; the pixels that cover it opaquely do not care: 0 * NaN is NaN
    got, _ = run(p, F.COMBOS[0], ((nan, 0.0, 1.0, 1.0), (nan, 0.0, 1.0, 1.0)), False)
    want, _ = compose_oracle.compose(rgba, bg_bottom=(nan, 0.0, 1.0, 1.0), bg_top=(nan, 0.0, 1.0, 1.0), srgb=False)
    np.testing.assert_array_equal(got, want)
    assert (got[0, :, 0] == 0).all()


def test_out_given_comes_back_and_nothing_outside_it_is_written():
    name, seed, h, w, bg = F.FAMILIES[3]
    p = F.planes(seed, h, w)
    pad = 64
    buf = torch.full((pad + h * w * 4 + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[pad:pad + h * w * 4].view(h, w, 4)
    kw = F.combo_args(p, F.COMBOS[2])
    res = RenderResult(dev(p["rgba"]), dev(kw["depth"]), None, dev(kw["flags"]), None)
    z = dev(kw["zbuf"])
    back = compose(volume(), res, background=bg, depth_buffer=z, srgb=False, out=out)
    torch.cuda.synchronize()
    assert back is out
    want, _ = compose_oracle.compose(p["rgba"], bg_bottom=bg[0], bg_top=bg[1], srgb=False, **kw)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + h * w * 4:] == 0xA5).all())


def test_refusals_launch_nothing_and_empty_frames_write_nothing():
    lib, vol = N.lib(), volume()
    h, w = 16, 24
    p = F.planes(3, h, w)
    # planes inside larger buffers, so that a pointer moved by one element still points into an allocation
    rgba_buf = torch.zeros(h * w * 4 + 8, dtype=torch.float32, device="cuda")
    rgba_buf[:h * w * 4] = dev(p["rgba"]).reshape(-1)
    out_buf = torch.full((h * w * 4 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    depth, flags = dev(p["depth"]), dev(p["flags"])
    zbuf = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
    assert rgba_buf.data_ptr() % 16 == 0 and out_buf.data_ptr() % 4 == 0
    q = N.ComposeParams()
    q.bg_bottom[:], q.bg_top[:], q.srgb_encode = (0.1, 0.2, 0.3, 1.0), (0.3, 0.2, 0.1, 1.0), 1
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                           # noqa: E731

    def call(ctx=vol._rings.handle, rgba=ptr(rgba_buf), d=ptr(depth), f=ptr(flags), width=w, height=h, params=C.byref(q),
             o=ptr(out_buf), z=ptr(zbuf)):
        return lib.svr_compose(ctx, rgba, d, f, width, height, params, o, z, None)

    cases = [
        (dict(ctx=None), "null argument"),
        (dict(rgba=None), "null argument"),
        (dict(params=None), "null argument"),
        (dict(o=None), "null argument"),
        (dict(width=-1), "negative size"),
        (dict(height=-3), "negative size"),
        (dict(d=None), "a depth test needs the render's depth plane"),
        (dict(rgba=ptr(rgba_buf, 4)), "rgba must be 16-byte aligned"),
        (dict(rgba=ptr(rgba_buf, 8)), "rgba must be 16-byte aligned"),
        (dict(o=ptr(out_buf, 1)), "out_rgba8 must be 4-byte aligned"),
        (dict(o=ptr(out_buf, 2)), "out_rgba8 must be 4-byte aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert ("svr_compose: " + msg) in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    # empty frames are accepted and write nothing
    assert call(width=0) == 0 and call(height=0) == 0 and call(width=0, height=0) == 0
    torch.cuda.synchronize()
    assert bool((out_buf == 0xA5).all()) and bool((zbuf == 7.0).all())              # nothing was launched
    assert call() == 0                                                              # the control case runs
    torch.cuda.synchronize()
    want, zwant = compose_oracle.compose(p["rgba"], p["depth"], p["flags"], tuple(q.bg_bottom), tuple(q.bg_top),
                                         zbuf=np.full((h, w), 7.0, np.float32), srgb=False)
    np.testing.assert_array_equal(out_buf[:h * w * 4].view(h, w, 4).cpu().numpy()[..., 3], want[..., 3])
    np.testing.assert_array_equal(zbuf.cpu().numpy(), zwant)
    assert bool((out_buf[h * w * 4:] == 0xA5).all()) and int((zbuf != 7.0).sum()) > 100

    # the Python surface: planes that are not what the kernel indexes are refused, not composed wrongly
    rgba = rgba_buf[:h * w * 4].view(h, w, 4)
    good = RenderResult(rgba, depth, None, flags, None)
    wide = lambda t: torch.cat([t, t], dim=1)                                       # noqa: E731
    crop = lambda t: wide(t)[:, :w]                                                 # a cropped view: right shape, wrong strides  # noqa: E731
    assert not crop(rgba).is_contiguous() and crop(rgba).shape == rgba.shape
    bad_results = [RenderResult(crop(rgba), depth, None, flags, None), RenderResult(rgba, crop(depth), None, flags, None),
                   RenderResult(rgba, depth, None, crop(flags), None),
                   RenderResult(rgba_buf[1:1 + h * w * 4].view(h, w, 4), depth, None, flags, None),      # 4-byte aligned
                   RenderResult(rgba, depth[:-1], None, flags, None), RenderResult(rgba, depth, None, flags.to(torch.int32), None)]
    assert bad_results[3].rgba.is_contiguous() and bad_results[3].rgba.data_ptr() % 16 == 4
    for bad in bad_results:
        with pytest.raises(ValueError):
            compose(vol, bad, depth_buffer=zbuf)
    for kw in (dict(out=crop(torch.empty((h, w, 4), dtype=torch.uint8, device="cuda"))),
               dict(out=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")),
               dict(depth_buffer=crop(zbuf)), dict(depth_buffer=zbuf.double())):
        with pytest.raises(ValueError):
            compose(vol, good, **kw)
    with pytest.raises(ValueError):
        compose(vol, RenderResult(rgba, None, None, flags, None), depth_buffer=zbuf)
    torch.cuda.synchronize()
    ok = compose(vol, good, background=(tuple(q.bg_bottom), tuple(q.bg_top)), srgb=False)      # and the control case
    torch.cuda.synchronize()
    want, _ = compose_oracle.compose(p["rgba"], None, p["flags"], tuple(q.bg_bottom), tuple(q.bg_top), srgb=False)
    np.testing.assert_array_equal(ok.cpu().numpy(), want)
