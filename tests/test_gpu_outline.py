"""GPU: svr_outline (include/svr.h) == the numpy restatement of tests/test_outline.py, bit for bit, on real renders:
64^3 synthetic scenes seen from outside (K1) and inside (K2) at 150 x 90 and 97 x 61, the 480^2 multi-scale demo
scene, one 1920 x 1080 frame; in place == out of place; a frame rendered as 2 x 2 regions and assembled == the
full frame; every host-side refusal of the C entry point, with nothing launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from sub_volume_renderer_amd import FrameRegion, RenderResult, _native as N, outline, testing
from test_outline import HIT, outline_reference, window_differs

pytestmark = pytest.mark.gpu

FRAMES = {
    "k1_150x90": dict(width=150, height=90, inside=False),
    "k2_150x90": dict(width=150, height=90, inside=True),
    "k1_97x61": dict(width=97, height=61, inside=False),
    "k2_97x61": dict(width=97, height=61, inside=True),
    "demo_480": None,
}
_scenes = {}


def scene_of(name):
    """(scene, planes of one render cloned off the volume's reusable outputs, host copies of them)."""
    if name not in _scenes:
        kw = FRAMES.get(name)
        if name == "demo_480":
            scene = testing.make_multiscale_demo_scene(480, 480)
        elif name == "k1_1920x1080":
            scene = testing.build(testing.synthetic_spec(64, 1920, 1080))
        else:
            scene = testing.build(testing.synthetic_spec(64, kw["width"], kw["height"], inside=kw["inside"]))
        r = scene.volume.render(scene.camera, scene.width, scene.height)
        res = RenderResult(r.rgba.clone(), r.depth.clone(), r.label.clone(), r.flags.clone(), None)
        torch.cuda.synchronize()
        host = dict(rgba=res.rgba.cpu().numpy(), depth=res.depth.cpu().numpy(), label=res.label.cpu().numpy(),
                    flags=res.flags.cpu().numpy())
        assert int((host["flags"] == HIT).sum()) > 100, "the frame has too few hits to test outlines"
        # a depth tolerance that separates some horizontally adjacent hits of one label: the 90th percentile of
        # their depth steps
        hit, lab, z = host["flags"] == HIT, host["label"], host["depth"]
        pair = hit[:, 1:] & hit[:, :-1] & (lab[:, 1:] == lab[:, :-1])
        steps = np.abs(z[:, 1:] - z[:, :-1])[pair]
        host["tau"] = float(np.quantile(steps, 0.9)) if steps.size else 0.0
        _scenes[name] = (scene, res, host)
    return _scenes[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_and_check(scene, res, host, *, near=None, **kw):
    """outline on the device vs outline_reference on the host copies; returns the edge count.  A selection given as
    a numpy array goes to the device as a tensor, to the restatement as a list."""
    sel = kw.get("selected")
    if isinstance(sel, np.ndarray):
        kw["selected"], sel = torch.from_numpy(sel).to(res.rgba.device), sel.tolist()
    mask = torch.full(res.flags.shape, 7, dtype=torch.uint8, device=res.rgba.device)
    got = outline(scene.volume, res, edge_mask=mask, **kw)
    torch.cuda.synchronize()
    want, want_mask = outline_reference(
        host["rgba"], host["label"], host["flags"], radius=kw.get("width", 1), depth=host["depth"],
        depth_tolerance=kw.get("depth_tolerance"), color=kw.get("color", (0, 0, 0, 1)),
        color_by_label=kw.get("color_by_label", False), colors=scene.volume.material._u["colors"], selected=sel,
        dim_unselected=kw.get("dim_unselected", 1.0), only_selected=kw.get("only_selected", False), near=near)
    g, m = got.cpu().numpy(), mask.cpu().numpy()
    np.testing.assert_array_equal(m, want_mask, err_msg=f"edge mask {kw}")
    np.testing.assert_array_equal(bits(g), bits(want), err_msg=f"rgba {kw}")
    miss = host["flags"] != HIT
    np.testing.assert_array_equal(bits(g[miss]), bits(host["rgba"][miss]))       # non-hits: the input, bit for bit
    return int(m.sum())


def selections(host):
    """empty, three labels of the frame, 100 000 random ids plus every label of the frame"""
    labels = host["label"].view(np.uint32)[host["flags"] == HIT]
    ids, counts = np.unique(labels, return_counts=True)
    three = [int(v) for v in ids[np.argsort(-counts, kind="stable")[:3]]]
    rng = np.random.default_rng(11)
    big = np.concatenate([rng.integers(0, 2**32, 100_000, dtype=np.uint64), ids.astype(np.uint64)]).astype(np.int64)
    return [None, three, big]


@pytest.mark.parametrize("depth_test", [False, True], ids=["z_off", "z_on"])
@pytest.mark.parametrize("radius", [1, 2, 5, 16])
@pytest.mark.parametrize("name", list(FRAMES))
def test_outline_matches_restatement(name, radius, depth_test):
    scene, res, host = scene_of(name)
    tau = host["tau"] if depth_test else None
    near = window_differs(host["label"], host["flags"], radius, host["depth"], tau)
    edges = []
    for by_label in (False, True):
        for sel in selections(host):
            for dim in (1.0, 0.25):
                for only in (False, True):
                    edges.append(run_and_check(scene, res, host, near=near, width=radius, depth_tolerance=tau,
                                               color=(0.9, 0.2, 0.1, 0.8), color_by_label=by_label, selected=sel,
                                               dim_unselected=dim, only_selected=only))
    assert max(edges) > 20
    # in place (out = the rgba plane of a copy) == out of place
    copy = RenderResult(res.rgba.clone(), res.depth, res.label, res.flags, None)
    kw = dict(width=radius, depth_tolerance=tau, color_by_label=True, selected=selections(host)[1], dim_unselected=0.25)
    ref = outline(scene.volume, res, **kw)
    back = outline(scene.volume, copy, out=copy.rgba, **kw)
    torch.cuda.synchronize()
    assert back.data_ptr() == copy.rgba.data_ptr()
    np.testing.assert_array_equal(bits(copy.rgba.cpu().numpy()), bits(ref.cpu().numpy()))


@pytest.mark.parametrize("radius", [16, 1])
def test_full_hd_frame(radius):
    """1920 x 1080 (60 x 135 workgroup tiles of 32 x 8): halos that cross tile edges everywhere and are clipped at
    every image border (the ragged last tiles are the 97 x 61 and 150 x 90 frames')."""
    scene, res, host = scene_of("k1_1920x1080")
    tau = host["tau"] if radius == 16 else None
    n = run_and_check(scene, res, host, width=radius, depth_tolerance=tau, color_by_label=radius == 16,
                      selected=selections(host)[1], dim_unselected=0.5)
    assert n > 20


def test_regions_assembled_then_outlined_equal_the_full_frame():
    scene, res, host = scene_of("k1_150x90")
    w, h = scene.width, scene.height
    full = {k: np.zeros_like(host[k]) for k in ("rgba", "depth", "label", "flags")}
    for x0, x1 in ((0, 64), (64, w)):
        for y0, y1 in ((0, 40), (40, h)):
            r = scene.volume.render(scene.camera, w, h, region=FrameRegion.tile(x0, y0, x1 - x0, y1 - y0))
            torch.cuda.synchronize()
            for k in full:
                full[k][y0:y1, x0:x1] = getattr(r, k).cpu().numpy()
    for k in full:                                              # the render itself does not depend on the tiling
        np.testing.assert_array_equal(full[k].view(np.uint8), host[k].view(np.uint8))
    dev = res.rgba.device
    assembled = RenderResult(*(torch.from_numpy(full[k]).to(dev) for k in ("rgba", "depth", "label", "flags")), None)
    kw = dict(width=2, depth_tolerance=host["tau"], color_by_label=True, selected=selections(host)[1], dim_unselected=0.25)
    a = outline(scene.volume, assembled, **kw)
    b = outline(scene.volume, res, **kw)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    assert int(((a != res.rgba).any(-1)).sum()) > 20


def test_host_validation_refuses_and_launches_nothing():
    scene, res, host = scene_of("k1_97x61")
    h, w = res.flags.shape
    lib = N.lib()
    out = torch.full_like(res.rgba, 7.0)
    mask = torch.full(res.flags.shape, 9, dtype=torch.uint8, device=res.rgba.device)
    colors = torch.ones((4, 4), dtype=torch.float32, device=res.rgba.device)
    sel = torch.zeros(3, dtype=torch.int32, device=res.rgba.device)
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731

    def params(**kw):
        q = N.OutlineParams(radius=1, depth_tolerance=-1.0, color_by_label=0, dim_unselected=1.0, only_selected=0)
        q.color[:] = (0.0, 0.0, 0.0, 1.0)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def call(q=None, rgba=p(res.rgba), depth=p(res.depth), label=p(res.label), flags=p(res.flags), width=w, height=h,
             cols=None, ncols=0, selected=None, nsel=0, o=p(out)):
        qp = C.byref(q) if q is not None else None
        return lib.svr_outline(scene.volume._rings.handle, rgba, depth, label, flags, width, height, qp, cols, ncols,
                               selected, nsel, o, p(mask), None)

    cases = [
        (dict(rgba=None, q=params()), "null argument"),
        (dict(label=None, q=params()), "null argument"),
        (dict(flags=None, q=params()), "null argument"),
        (dict(o=None, q=params()), "null argument"),
        (dict(q=None), "null argument"),
        (dict(width=-1, q=params()), "negative size"),
        (dict(height=-5, q=params()), "negative size"),
        (dict(q=params(radius=0)), "radius must be in [1, 16]"),
        (dict(q=params(radius=17)), "radius must be in [1, 16]"),
        (dict(depth=None, q=params(depth_tolerance=0.0)), "needs the render's depth plane"),
        (dict(q=params(color_by_label=1)), "color_by_label needs at least one color"),
        (dict(cols=p(colors), ncols=0, q=params(color_by_label=1)), "color_by_label needs at least one color"),
        (dict(q=params(color=(C.c_float * 4)(0, 0, 0, 1.5))), "opacity color[3] must be in [0, 1]"),
        (dict(q=params(color=(C.c_float * 4)(0, 0, 0, -0.1))), "opacity color[3] must be in [0, 1]"),
        (dict(q=params(dim_unselected=1.5)), "dim_unselected must be in [0, 1]"),
        (dict(q=params(dim_unselected=-0.5)), "dim_unselected must be in [0, 1]"),
        (dict(nsel=3, q=params()), "selected_count > 0 with a NULL selected pointer"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (kw, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mask == 9).all())         # nothing was launched
    assert call(q=params(), cols=p(colors), ncols=4, selected=p(sel), nsel=3) == 0     # the control case runs
    torch.cuda.synchronize()
    assert not bool((mask == 9).any()) and int(mask.sum()) > 20
    # the Python surface refuses the same things before the C entry point
    for bad in (dict(width=0), dict(width=17), dict(color=(0, 0, 0, 2)), dict(dim_unselected=-1), dict(depth_tolerance=-1),
                dict(out=torch.empty((h, w, 3), device=res.rgba.device))):
        with pytest.raises(ValueError):
            outline(scene.volume, res, **bad)
    with pytest.raises(ValueError):
        outline(scene.volume, RenderResult(res.rgba, None, res.label, res.flags, None), depth_tolerance=0.1)
