"""GPU: svr_outline (include/svr.h) == the numpy restatement of tests/test_outline.py, bit for bit, on the hand-made and
seeded families of tests/outline_cases.py — the inputs real renders never hold: one odd pixel on tile seams and image
corners, frames smaller than a tile or the halo, labels 0 and 0xFFFFFFFF, labels >= 2^31 under a palette whose length
is no power of two, infinite / NaN / signed-zero depths, a depth step of exactly the tolerance, tolerances 0, -0 and
+inf, opacity 0 and 1, NaN / inf / subnormal RGBA, flag bytes 3 and 255, selections handed to the C entry point as they
are.  Outputs start as sentinels; a NaN channel compares as NaN, everything else as bits."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import outline_cases as OC
from sub_volume_renderer_amd import RenderResult, _native as N, outline
from sub_volume_renderer_amd._wrapping_buffer import DeviceRings
from test_outline import HIT, window_differs

pytestmark = pytest.mark.gpu

SENTINEL_RGBA, SENTINEL_MASK = -7777.0, 7


class _Volume:
    """What `outline()` reads of a volume: the context and the material's colour table."""

    def __init__(self):
        self._rings = DeviceRings([(4, 4, 8)], labels=False)
        self.material = None

    def with_colors(self, colors):
        table = np.zeros((1, 4), np.float32) if colors is None else np.asarray(colors, np.float32)
        self.material = types.SimpleNamespace(_u={"colors": table}, _version=0)      # a new object: the cached table is rebuilt
        return self


_volume = None


def volume():
    global _volume
    if _volume is None:
        _volume = _Volume()
    return _volume


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def params_of(kw):
    tau = kw.get("depth_tolerance")
    q = N.OutlineParams(radius=kw["radius"], depth_tolerance=-1.0 if tau is None else tau,
                        color_by_label=1 if kw.get("color_by_label") else 0,
                        dim_unselected=kw.get("dim_unselected", 1.0), only_selected=1 if kw.get("only_selected") else 0)
    q.color[:] = kw.get("color", (0, 0, 0, 1))
    return q


def run(case, *, in_place=False, null_mask=False):
    """The kernel's (rgba, edge mask or None) for one case: through `outline()` where Python's checks let the inputs
    pass unchanged, else through svr_outline itself."""
    dev = torch.device("cuda")
    kw = case.kwargs
    h, w = case.flags.shape
    rgba = torch.from_numpy(case.rgba).to(dev)
    depth = torch.from_numpy(case.depth).to(dev)
    label = torch.from_numpy(case.label.view(np.int32)).to(dev)
    flags = torch.from_numpy(case.flags).to(dev)
    out = rgba if in_place else torch.full_like(rgba, SENTINEL_RGBA)
    mask = None if null_mask else torch.full((h, w), SENTINEL_MASK, dtype=torch.uint8, device=dev)
    vol = volume().with_colors(kw.get("colors"))
    if case.direct:
        colors = torch.from_numpy(np.ascontiguousarray(kw["colors"], np.float32)).to(dev) if kw.get("color_by_label") else None
        sel = kw.get("selected")
        sel = torch.from_numpy(np.asarray(sel, np.uint32).view(np.int32)).to(dev) if sel is not None and len(sel) else None
        q = params_of(kw)
        rc = N.lib().svr_outline(vol._rings.handle, ptr(rgba), ptr(depth), ptr(label), ptr(flags), w, h, C.byref(q),
                                 ptr(colors), 0 if colors is None else colors.shape[0], ptr(sel),
                                 0 if sel is None else sel.numel(), ptr(out), ptr(mask), None)
        assert rc == 0, N.lib().svr_last_error()
    else:
        sel = kw.get("selected")
        got = outline(vol, RenderResult(rgba, depth, label, flags, None), width=kw["radius"],
                      color=kw.get("color", (0, 0, 0, 1)), color_by_label=bool(kw.get("color_by_label")),
                      depth_tolerance=kw.get("depth_tolerance"), selected=None if sel is None else [int(v) for v in sel],
                      dim_unselected=kw.get("dim_unselected", 1.0), only_selected=bool(kw.get("only_selected")), out=out,
                      edge_mask=mask)
        assert got is out
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if mask is None else mask.cpu().numpy()


def assert_rgba(got, want, msg):
    """u32 bits, except that a NaN of the restatement is met by any NaN (payloads are not part of the definition)."""
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{msg}: {np.count_nonzero(~same)} channels differ, first at {np.argwhere(~same)[:4].tolist()}"


def hold(case, near=None, in_place=False):
    """One case against the restatement (and its closed form); returns the edge count."""
    want, want_mask = OC.reference(case, near)
    got, mask = run(case)
    np.testing.assert_array_equal(mask, want_mask, err_msg=f"edge mask {case.name}")
    if case.mask is not None:
        np.testing.assert_array_equal(mask, case.mask, err_msg=f"closed form {case.name}")
    assert_rgba(got, want, case.name)
    miss = case.flags != HIT
    np.testing.assert_array_equal(bits(got[miss]), bits(case.rgba[miss]), err_msg=f"non-hits {case.name}")
    plain, none = run(case, null_mask=True)                             # edge_mask = NULL: the same RGBA
    assert none is None
    np.testing.assert_array_equal(bits(plain), bits(got), err_msg=f"NULL edge mask {case.name}")
    if in_place:
        back, mask2 = run(case, in_place=True)
        np.testing.assert_array_equal(bits(back), bits(got), err_msg=f"in place {case.name}")
        np.testing.assert_array_equal(mask2, mask)
    return int(mask.sum())


@pytest.mark.parametrize("kind", list(OC.LONE_KINDS))
def test_lone_pixel(kind):
    cases = list(OC.lone_pixel_cases([kind]))
    assert len(cases) == 13 * len(OC.LONE_FRAMES)
    assert all(c.direct == (kind in ("flag3", "flag255")) for c in cases)
    for case in cases:
        assert hold(case) == int(case.mask.sum()) >= 3


def hold_frames(frames, family):
    total = 0
    for name, planes, r, tau, cases in OC.frame_cases(frames, family):
        rgba, depth, label, flags, _ = planes
        near = window_differs(label, flags, r, depth, tau)
        for case in cases:
            total += hold(case, near=near, in_place=True)
    return total


@pytest.mark.parametrize("size", OC.TINY_FRAMES, ids=lambda s: "%dx%d" % s)
def test_tiny_and_ragged_frames(size):
    frames = [f for f in OC.tiny_frames() if f[1][3].shape == size[::-1]]
    assert len(frames) == (2 if size == (5, 3) else 2 * len(OC.TINY_RADII))
    edges = hold_frames(frames, "tiny")
    assert edges > 0 or size == (1, 1)


@pytest.mark.parametrize("frame", range(len(OC.BLOCKY_FRAMES)), ids=["%dx%d-r%d" % f for f in OC.BLOCKY_FRAMES])
def test_blocky_frames(frame):
    # (the census of test_outline.py: at least 50 edges with the depth test on and off, in the two variants that outline all)
    assert hold_frames(OC.blocky_frames([OC.BLOCKY_FRAMES[frame]]), "blocky") > 4 * 50


@pytest.mark.parametrize("radius", OC.DEPTH_RADII)
def test_depth_family(radius):
    cases = list(OC.depth_cases([radius]))
    assert any(c.direct for c in cases) and any(not c.direct for c in cases)        # -0.0 goes to the C entry point
    drawn = sum(hold(case) > 0 for case in cases)
    assert len(cases) // 4 < drawn < 3 * len(cases) // 4


def test_hand_written_rows():
    for case in OC.hand_cases():
        hold(case)


def test_colour_family():
    cases = list(OC.color_cases())
    assert len(cases) == 3 + 2 + 4 + 3 + 3
    for case in cases:
        assert hold(case, in_place=True) > 0


def test_selections_through_the_c_entry_point():
    cases = list(OC.selection_cases())
    assert all(c.direct for c in cases) and {len(c.kwargs["selected"]) for c in cases} >= {1, 2, 3, 1000}
    near = {}
    for case in cases:
        key = case.name.split("-")[1]
        if key not in near:
            near[key] = window_differs(case.label, case.flags, case.kwargs["radius"], case.depth, case.kwargs["depth_tolerance"])
        edges = hold(case, near=near[key])
        assert edges > 50 or case.kwargs["only_selected"]               # (an id that no pixel holds outlines nothing)


def test_refusals_not_asserted_elsewhere():
    """A NaN tolerance, and rgba, out_rgba or colors off 16-byte alignment: each returns SVR_ERR_INVALID, leaves its
    message, and launches nothing; then the control call runs."""
    dev = torch.device("cuda")
    case = next(OC.cases_of_frame(*next(OC.blocky_frames([(70, 41, 2)])), "blocky"))
    h, w = case.flags.shape
    lib = N.lib()
    handle = volume()._rings.handle

    def shifted(a, dtype=torch.float32):
        """(the array 4 bytes past a 16-byte boundary, the same aligned)"""
        flat = torch.zeros(a.size + 4, dtype=dtype, device=dev)
        assert flat.data_ptr() % 16 == 0
        flat[1:1 + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
        return flat[1:1 + a.size]

    rgba = torch.from_numpy(case.rgba).to(dev)
    depth = torch.from_numpy(case.depth).to(dev)
    label = torch.from_numpy(case.label.view(np.int32)).to(dev)
    flags = torch.from_numpy(case.flags).to(dev)
    pal = OC.palette(OC.PALETTE7)
    colors = torch.from_numpy(pal).to(dev)
    rgba_off, colors_off = shifted(case.rgba), shifted(pal)
    out_room = torch.full((h * w * 4 + 4,), SENTINEL_RGBA, dtype=torch.float32, device=dev)
    out = out_room[:h * w * 4]
    mask = torch.full((h, w), SENTINEL_MASK, dtype=torch.uint8, device=dev)
    assert rgba.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and colors.data_ptr() % 16 == 0
    assert rgba_off.data_ptr() % 16 == 4 and colors_off.data_ptr() % 16 == 4

    def call(tau=0.001, by_label=1, rgba_=rgba, out_=out, colors_=colors):
        q = params_of(dict(radius=2, depth_tolerance=tau, color=OC.COLOR, color_by_label=by_label))
        return lib.svr_outline(handle, ptr(rgba_), ptr(depth), ptr(label), ptr(flags), w, h, C.byref(q), ptr(colors_), 7,
                               None, 0, ptr(out_), ptr(mask), None)

    refused = [(dict(tau=float("nan")), "svr_outline: depth_tolerance is NaN"),
               (dict(rgba_=rgba_off), "svr_outline: rgba, out_rgba and colors must be 16-byte aligned"),
               (dict(out_=out_room[1:]), "svr_outline: rgba, out_rgba and colors must be 16-byte aligned"),
               (dict(colors_=colors_off), "svr_outline: rgba, out_rgba and colors must be 16-byte aligned")]
    for kw, msg in refused:
        assert call(**kw) == -1, kw
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((out_room == SENTINEL_RGBA).all()) and bool((mask == SENTINEL_MASK).all())      # nothing was launched
    assert call() == 0, lib.svr_last_error()
    torch.cuda.synchronize()
    want, want_mask = OC.reference(OC.Case("control", case.rgba, case.depth, case.label, case.flags,
                                           dict(radius=2, depth_tolerance=0.001, color=OC.COLOR, color_by_label=True, colors=pal)))
    np.testing.assert_array_equal(mask.cpu().numpy(), want_mask)
    assert_rgba(out.cpu().numpy().reshape(h, w, 4), want, "control")
    assert float(out_room[-1]) == SENTINEL_RGBA
