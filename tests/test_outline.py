"""Segmentation outlines (svr_outline, include/svr.h) on the CPU: an independent numpy float32 restatement of the
definition in the header, held to hand-made planes with hand-written answers; the C struct and the host-side
refusal of a NULL context.  tests/test_gpu_outline.py holds the HIP kernel to this restatement bit for bit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from sub_volume_renderer_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HIT, MISS, DISCARD = 2, 1, 0


def hsv_to_rgb_reference(h, s, v):
    """hsv_selection.wgsl:7-41 on float32 arrays, the sector by the floor of h * 6 (NaN / out-of-range: last branch)."""
    h, s = np.asarray(h, F32), np.asarray(s, F32)
    v = np.broadcast_to(F32(v), h.shape)
    with np.errstate(invalid="ignore"):
        hs = h * F32(6)
        fl = np.floor(hs)
        fr = hs - fl
        p = v * (F32(1) - s)
        q = v * (F32(1) - s * fr)
        t = v * (F32(1) - s * (F32(1) - fr))
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v)]
    out = np.stack([v, p, q], -1)                                    # else branch
    for k in range(4, -1, -1):
        out = np.where((fl == F32(k))[..., None], np.stack(table[k], -1), out)
    return np.where((s == F32(0))[..., None], np.stack([v, v, v], -1), out).astype(F32)


def window_differs(label, flags, radius, depth=None, depth_tolerance=None):
    """Per pixel: some q in N_r(p) is a non-hit, a hit of another label, or (tolerance given) a hit whose depth is
    more than the tolerance away (include/svr.h, svr_outline), tested neighbour by neighbour."""
    flags = np.asarray(flags)
    lab = np.asarray(label).view(np.uint32) if np.asarray(label).dtype == np.int32 else np.asarray(label, np.uint32)
    h, w = flags.shape
    hit = flags == HIT
    if depth_tolerance is not None:
        z, tau = np.asarray(depth, F32), F32(depth_tolerance)
    near = np.zeros((h, w), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            # p over the pixels whose neighbour q = p + (dy, dx) lies inside the image
            py, qy = slice(max(0, -dy), min(h, h - dy)), slice(max(0, dy), min(h, h + dy))
            px, qx = slice(max(0, -dx), min(w, w - dx)), slice(max(0, dx), min(w, w + dx))
            hq = hit[qy, qx]
            d = ~hq | (lab[qy, qx] != lab[py, px])
            if depth_tolerance is not None:
                with np.errstate(invalid="ignore"):
                    d |= hq & (np.abs(z[qy, qx] - z[py, px]) > tau)
            near[py, px] |= d
    return near


def outline_reference(rgba, label, flags, *, radius, depth=None, depth_tolerance=None, color=(0, 0, 0, 1),
                      color_by_label=False, colors=None, selected=None, dim_unselected=1.0, only_selected=False,
                      near=None):
    """The definition in include/svr.h.  Returns (out f32 [h, w, 4], edge_mask u8 [h, w]).  ``near``: the
    `window_differs` of these planes, radius and tolerance, when the caller already has it."""
    rgba = np.asarray(rgba, F32)
    flags = np.asarray(flags)
    lab = np.asarray(label).astype(np.int64) & 0xFFFFFFFF
    h, w = flags.shape
    hit = flags == HIT
    if near is None:
        near = window_differs(label, flags, radius, depth, depth_tolerance)
    sel_ids = np.unique(np.asarray(list(selected) if selected is not None else [], np.int64) & 0xFFFFFFFF)
    is_sel = np.isin(lab, sel_ids) if sel_ids.size else np.ones((h, w), bool)
    edge = hit & near & (is_sel if only_selected else True)
    b = rgba.copy()
    if sel_ids.size:
        dim = hit & ~is_sel
        b[dim, :3] = rgba[dim, :3] * F32(dim_unselected)
    if color_by_label:
        pal = np.asarray(colors, F32).reshape(-1, 4)
        hsv = pal[lab % pal.shape[0]]
        c = hsv_to_rgb_reference(hsv[..., 0], hsv[..., 1], 1.0)
    else:
        c = np.broadcast_to(np.asarray(color[:3], F32), (h, w, 3))
    a = F32(color[3])
    oma = F32(1) - a
    out = b.copy()
    out[edge, :3] = b[edge, :3] * oma + c[edge] * a
    out[edge, 3] = b[edge, 3] * oma + a
    out[~hit] = rgba[~hit]
    return out, edge.astype(np.uint8)


def rgba_of(flags, seed=0):
    rgba = np.random.default_rng(seed).random((*flags.shape, 4), dtype=F32)
    rgba[flags == MISS] = (0, 0, 0, 1)                              # what the march writes (fs_main.wgsl:93-98)
    rgba[flags == DISCARD] = 0
    return rgba


def two_labels_frame():
    """6 x 8: label 5 left of x = 4, label 9 on x = 4 .. 6, a miss at (2, 2), a discarded column x = 7."""
    flags = np.full((6, 8), HIT, np.uint8)
    flags[2, 2] = MISS
    flags[:, 7] = DISCARD
    label = np.where(np.arange(8)[None, :] < 4, 5, 9).repeat(6, 0).astype(np.int32)
    label[flags != HIT] = 0
    return rgba_of(flags), label, flags


EDGES_R1 = np.array([[0, 0, 0, 1, 1, 0, 1, 0],
                     [0, 1, 1, 1, 1, 0, 1, 0],
                     [0, 1, 0, 1, 1, 0, 1, 0],
                     [0, 1, 1, 1, 1, 0, 1, 0],
                     [0, 0, 0, 1, 1, 0, 1, 0],
                     [0, 0, 0, 1, 1, 0, 1, 0]], np.uint8)
EDGES_R2 = np.array([[1, 1, 1, 1, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1, 1, 1, 0],
                     [1, 1, 0, 1, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1, 1, 1, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0]], np.uint8)


@pytest.mark.parametrize("radius, want", [(1, EDGES_R1), (2, EDGES_R2)])
def test_hand_made_frame(radius, want):
    rgba, label, flags = two_labels_frame()
    color = (0.25, 0.5, 1.0, 0.75)
    out, mask = outline_reference(rgba, label, flags, radius=radius, color=color)
    np.testing.assert_array_equal(mask, want)
    e = want.astype(bool)
    np.testing.assert_array_equal(out[~e], rgba[~e])                # no selection: everything else untouched
    np.testing.assert_array_equal(out[e, :3], rgba[e, :3] * F32(0.25) + np.array(color[:3], F32) * F32(0.75))
    np.testing.assert_array_equal(out[e, 3], rgba[e, 3] * F32(0.25) + F32(0.75))


def test_image_border_draws_no_edge():
    flags = np.full((5, 7), HIT, np.uint8)
    label = np.full((5, 7), 3, np.int32)
    rgba = rgba_of(flags)
    for r in (1, 2, 16):
        out, mask = outline_reference(rgba, label, flags, radius=r)
        assert mask.sum() == 0
        np.testing.assert_array_equal(out, rgba)
    label[4, 6] = 4                                                 # one corner pixel of another label
    _, mask = outline_reference(rgba, label, flags, radius=1)
    want = np.zeros((5, 7), np.uint8)
    want[3:, 5:] = 1
    np.testing.assert_array_equal(mask, want)


def test_depth_tolerance_separates_parts_of_one_label():
    flags = np.full((4, 6), HIT, np.uint8)
    label = np.full((4, 6), 7, np.int32)
    z = np.where(np.arange(6)[None, :] < 3, F32(0.2), F32(0.5)).repeat(4, 0).astype(F32)
    rgba = rgba_of(flags)
    _, m = outline_reference(rgba, label, flags, radius=1, depth=z, depth_tolerance=0.25)
    want = np.zeros((4, 6), np.uint8)
    want[:, 2:4] = 1
    np.testing.assert_array_equal(m, want)
    for tau in (0.35, None):
        _, m = outline_reference(rgba, label, flags, radius=1, depth=z, depth_tolerance=tau)
        assert m.sum() == 0
    _, m = outline_reference(rgba, label, flags, radius=3, depth=z, depth_tolerance=0.25)
    np.testing.assert_array_equal(m, np.ones((4, 6), np.uint8))     # every pixel is within 3 of the step


def test_selection_dims_the_others_and_only_selected_outlines_it():
    rgba, label, flags = two_labels_frame()
    color = (1.0, 0.0, 0.0, 1.0)
    out, mask = outline_reference(rgba, label, flags, radius=1, color=color, selected=[5], dim_unselected=0.25)
    np.testing.assert_array_equal(mask, EDGES_R1)                  # the selection alone does not change the edges
    other = (label == 9) & (flags == HIT) & ~EDGES_R1.astype(bool)
    np.testing.assert_array_equal(out[other, :3], rgba[other, :3] * F32(0.25))
    np.testing.assert_array_equal(out[other, 3], rgba[other, 3])
    edge9 = (label == 9) & EDGES_R1.astype(bool)
    np.testing.assert_array_equal(out[edge9], np.broadcast_to(np.array(color, F32), out[edge9].shape))
    keep = (label == 5) & (flags == HIT) & ~EDGES_R1.astype(bool)
    np.testing.assert_array_equal(out[keep], rgba[keep])
    np.testing.assert_array_equal(out[flags != HIT], rgba[flags != HIT])
    out2, mask2 = outline_reference(rgba, label, flags, radius=1, color=color, selected=[5], dim_unselected=0.25,
                                    only_selected=True)
    np.testing.assert_array_equal(mask2, EDGES_R1 * (label == 5))
    np.testing.assert_array_equal(out2[label == 9][:, :3], rgba[label == 9][:, :3] * F32(0.25))   # dimmed, not outlined
    # an empty selection selects everything: only_selected changes nothing
    _, mask3 = outline_reference(rgba, label, flags, radius=1, selected=[], only_selected=True)
    np.testing.assert_array_equal(mask3, EDGES_R1)


def test_color_by_label_covers_every_hue_sector():
    hues = [(0.05, 0.5), (0.2, 0.5), (0.4, 0.5), (0.55, 0.5), (0.7, 0.5), (0.9, 0.5), (1.25, 0.5), (0.3, 0.0)]
    colors = np.array([(hh, s, 0.8, 1.0) for hh, s in hues], F32)   # v of the table is not used: the outline is at v = 1
    flags = np.full((1, 8), HIT, np.uint8)
    label = np.arange(8, dtype=np.int32)[None, :] + 8               # 8 + k -> colors[k]
    rgba = rgba_of(flags)
    out, mask = outline_reference(rgba, label, flags, radius=1, color_by_label=True, colors=colors)
    assert mask.all()
    s, fr = F32(0.5), lambda hh: F32(hh) * F32(6) - np.floor(F32(hh) * F32(6))
    p = F32(1) - s
    q = lambda hh: F32(1) - s * fr(hh)                              # noqa: E731
    t = lambda hh: F32(1) - s * (F32(1) - fr(hh))                   # noqa: E731
    want = [(1, t(0.05), p), (q(0.2), 1, p), (p, 1, t(0.4)), (p, q(0.55), 1), (t(0.7), p, 1), (1, p, q(0.9)),
            (1, p, q(1.25)),                                        # h >= 1: sector 7, the else branch (no wrap-around)
            (1, 1, 1)]                                              # s = 0: grey at v
    np.testing.assert_array_equal(out[0, :, :3], np.array(want, F32))
    np.testing.assert_array_equal(out[0, :, 3], np.ones(8, F32))
    assert out[0, 6, 1] == p and out[0, 6, 2] == F32(0.75)


def test_outline_params_struct_matches_the_header(tmp_path):
    fields = [name for name, _ in _native.OutlineParams._fields_]
    assert fields == ["radius", "depth_tolerance", "color_by_label", "color", "dim_unselected", "only_selected"]
    assert ctypes.sizeof(_native.OutlineParams) == 36
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler on this machine")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svr.h"\nint main(void) {\n'
                   + "".join(f'    printf("%zu\\n", offsetof(svr_outline_params, {f}));\n' for f in fields)
                   + '    printf("%zu\\n", sizeof(svr_outline_params));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [getattr(_native.OutlineParams, f).offset for f in fields] + [ctypes.sizeof(_native.OutlineParams)]
    assert got == want


def test_null_context_is_refused_with_a_message():
    lib = _native.lib()
    q = _native.OutlineParams(radius=1)
    q.color[3] = 1.0
    q.dim_unselected = 1.0
    assert lib.svr_outline(None, None, None, None, None, 8, 8, ctypes.byref(q), None, 0, None, 0, None, None, None) == -1
    assert b"svr_outline: null argument" in lib.svr_last_error()
    with pytest.raises(ValueError, match="svr_outline"):
        _native.check(lib.svr_outline(None, None, None, None, None, 8, 8, ctypes.byref(q), None, 0, None, 0, None,
                                      None, None), "svr_outline")
