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


# ---- the restatement at its edges (tests/outline_cases.py): answers that do not come from it --------------------------
import outline_cases as OC  # noqa: E402


@pytest.mark.parametrize("kind", list(OC.LONE_KINDS))
def test_lone_pixel_marks_its_chebyshev_ball(kind):
    """One odd pixel in a uniform frame, at the centre, the image corners and either side of the tile seams: the edge
    mask is the ball of radius r round it clipped to the image, with the pixel itself when it is a hit (labels 0 and
    0xFFFFFFFF included) and without it when its flag byte is anything else (0, 1, 3, 255)."""
    n = 0
    for case in OC.lone_pixel_cases([kind]):
        out, mask = OC.reference(case)
        np.testing.assert_array_equal(mask, case.mask, err_msg=case.name)
        assert int(case.mask.sum()) >= 3                                # a corner at r = 1 without its centre
        miss = case.flags != HIT
        np.testing.assert_array_equal(out[miss], case.rgba[miss])
        n += 1
    assert n == 13 * len(OC.LONE_FRAMES)


def test_strict_depth_step_values_are_exact():
    z0, tau, odd = OC.strict_step_values()
    assert (z0, tau) == (F32(0.0625), F32(0.125))
    assert odd["above_by_tau"] == (F32(0.1875), False) and odd["below_by_tau"] == (F32(-0.0625), False)
    assert float(odd["above_by_next"][0]) == 0.1875 + 2.0 ** -26 and odd["above_by_next"][1]
    assert float(odd["below_by_next"][0]) == -0.0625 - 2.0 ** -26 and odd["below_by_next"][1]     # one ulp of tau


@pytest.mark.parametrize("radius", OC.DEPTH_RADII)
def test_depth_family_against_scalar_arithmetic(radius):
    """A step of exactly tau draws nothing and the next f32 draws the ball, above and below the field; +-inf, NaN, signed
    zeros and a subnormal as field and as odd pixel under tau 0, -0, +inf and 1e-3 (a NaN on either side never
    differs; -0.0 turns the test on like 0.0); a non-hit's stale depth makes a silhouette and nothing else."""
    cases = list(OC.depth_cases([radius]))
    assert len(cases) == 4 + 36 * (2 if radius == 16 else 4) + 2
    edges = 0
    for case in cases:
        _, mask = OC.reference(case)
        np.testing.assert_array_equal(mask, case.mask, err_msg=case.name)
        edges += bool(case.mask.any())
    assert len(cases) // 4 < edges < 3 * len(cases) // 4               # both outcomes are well represented
    by_name = {c.name.rsplit("-r", 1)[0]: c for c in cases}
    ball = (2 * radius + 1) ** 2                                        # the odd pixel is further than 16 from every border
    assert by_name["depth-field+inf-odd+inf-tau-0"].mask.sum() == 0                # inf - inf is NaN: no step
    assert by_name["depth-field+inf-odd-inf-tau1e-3"].mask.sum() == ball
    assert by_name["depth-field-0-odd+0-tau-0"].mask.sum() == 0                    # |0 - -0| = 0 is not > -0
    assert by_name["depth-field+0-oddsubnormal-tau-0"].mask.sum() == ball
    assert by_name["depth-field+0-oddnan-tau1e-3"].mask.sum() == 0
    assert by_name["depth-field+0-oddsubnormal-tau-0"].direct and not by_name["depth-field+0-oddnan-tau1e-3"].direct
    if radius != 16:
        assert by_name["depth-field+inf-odd-inf-tau+inf"].mask.sum() == 0          # nothing exceeds +inf


def test_hand_written_rows():
    cases = list(OC.hand_cases())
    assert [c.name for c in cases][:2] == ["hand-1x1-r16", "hand-top-labels-inf-nan"]
    for case in cases:
        _, mask = OC.reference(case)
        np.testing.assert_array_equal(mask, case.mask, err_msg=case.name)


def test_label_modulo_is_unsigned():
    """0xFFFFFFFF % 3 = 0 and 0x80000000 % 3 = 2 (a signed 32-bit modulo gives -1 and -2); % 7: 3 and 2; % 1: 0."""
    assert [l % 3 for l in OC.MODULO_LABELS[:2]] == [0, 2] and [l % 7 for l in OC.MODULO_LABELS[:2]] == [3, 2]
    for case in OC.color_cases():
        if not case.name.startswith("color-modulo"):
            continue
        pal = case.kwargs["colors"]
        out, mask = OC.reference(case)
        np.testing.assert_array_equal(mask, case.mask)
        idx = [l % len(pal) for l in OC.MODULO_LABELS]                  # Python ints: no sign to get wrong
        want = hsv_to_rgb_reference(pal[idx, 0], pal[idx, 1], 1.0)      # opacity 1: the outline colour itself
        np.testing.assert_array_equal(out[0, :, :3], want)
        np.testing.assert_array_equal(out[1, :, :3], want)
        if len(pal) > 1:
            assert len({tuple(c) for c in want.tolist()}) == len(set(idx))    # the palette entries differ visibly


def test_hue_table_reaches_every_branch():
    """The hue / saturation table of the colour family: NaN only where the hue is NaN and the saturation is not 0;
    1/6 and its upper neighbour fall in sector 1, its lower neighbour in sector 0; 1.0, 1.25, -0.1 and 1e30 take the
    last branch."""
    h = np.array(OC.HUES, F32)
    fl = np.floor(h * F32(6))
    assert fl[:5].tolist() == [0.0, 0.0, 1.0, 1.0, 5.0] and fl[5:8].tolist() == [6.0, 7.0, -1.0] and fl[8] > 1e30
    for s in (0.5, 1.0):
        rgb = hsv_to_rgb_reference(h, np.full(h.shape, s, F32), 1.0)
        assert np.isnan(rgb[-1]).any() and not np.isnan(rgb[:-1]).any()
        assert rgb[1, 0] == 1 and rgb[2, 1] == 1 and rgb[3, 1] == 1                  # (v, t, p) then (q, v, p)
        np.testing.assert_array_equal(rgb[5:9, 0], np.ones(4, F32))                  # (v, p, q)
    assert not np.isnan(hsv_to_rgb_reference(h, np.zeros(h.shape, F32), 1.0)).any()


def test_opacity_dimming_and_pass_through_of_special_rgba():
    cases = {c.name: c for c in OC.color_cases()}
    for by in (0, 1):
        c = cases[f"color-opacity0-by{by}"]
        out, mask = OC.reference(c)
        assert mask.all()
        np.testing.assert_array_equal(out, c.rgba)                      # b * 1 + c * 0 on finite non-negative values
        c = cases[f"color-opacity1-by{by}"]
        out, _ = OC.reference(c)
        assert np.all(out[..., 3] == 1)
    c = cases["color-dim0.001-subnormal"]
    assert np.all(np.abs(c.rgba) < np.finfo(F32).tiny) and np.all(c.rgba != 0)
    sel = c.label == 2
    for name in ("color-dim0-subnormal", "color-dim1-subnormal", "color-dim0.001-subnormal"):
        c = cases[name]
        out, mask = OC.reference(c)
        quiet = ~sel & ~mask.astype(bool)
        assert quiet.any()
        np.testing.assert_array_equal(out[quiet][:, :3].view(np.uint32),
                                      (c.rgba[quiet][:, :3] * F32(c.kwargs["dim_unselected"])).view(np.uint32))
    c = cases["color-special-rgba-a0.5"]
    out, _ = OC.reference(c)
    miss = c.flags != HIT
    assert miss.sum() >= 20 and np.isnan(c.rgba[miss]).any() and np.isinf(c.rgba[miss]).any()
    np.testing.assert_array_equal(out[miss].view(np.uint32), c.rgba[miss].view(np.uint32))


def test_no_blocky_frame_is_vacuous():
    """For every (family-5 frame, r, depth test on / off) the restatement's mask holds at least 50 edge hits and at least
    50 hits that are no edge; the frames hold labels 0 and 0xFFFFFFFF as hits and flag bytes 0, 1, 2 and 3."""
    frames = list(OC.blocky_frames())
    assert len(frames) == 2 * len(OC.BLOCKY_FRAMES)
    for name, (rgba, depth, label, flags, tau_on), r, tau in frames:
        hit = flags == HIT
        near = window_differs(label, flags, r, depth, tau)
        assert int((hit & near).sum()) >= 50 and int((hit & ~near).sum()) >= 50, name
        assert 0.75 < hit.mean() < 0.95 and set(np.unique(flags)) == {0, 1, 2, 3}, name
        assert (label[hit] == 0).any() and (label[hit] == OC.TOP).any(), name
        if tau is not None:
            assert tau > 0 and int((near & ~window_differs(label, flags, r)).sum()) >= 20, name      # the depth test adds edges
    for name, planes, r, tau in OC.tiny_frames():
        assert planes[3].shape in {(h, w) for w, h in OC.TINY_FRAMES}
    sizes = {(c.flags.shape, c.kwargs["radius"]) for c in OC.frame_cases(OC.tiny_frames(), "tiny")[0][4]}
    assert sizes == {((1, 1), 1)}


def test_selection_family_is_sorted_and_reaches_both_ends():
    cases = list(OC.selection_cases())
    lens = {len(c.kwargs["selected"]) for c in cases}
    assert {1, 2, 3, 1000} <= lens and all(c.direct for c in cases)
    changed = 0
    for c in cases:
        sel = c.kwargs["selected"]
        assert sel.dtype == np.uint32 and np.all(sel[1:] >= sel[:-1])
        out, mask = OC.reference(c)
        hit = c.flags == HIT
        dimmed = hit & ~np.isin(c.label, sel)
        assert dimmed.any()                                             # no selection holds every label of its frame
        changed += int(np.isin(c.label[hit], sel).any())
    mid = [c for c in cases if "-mid-" in c.name]
    lo, hi = mid[0].label[mid[0].flags == HIT].min(), mid[0].label[mid[0].flags == HIT].max()
    assert any(c.kwargs["selected"][0] < lo and c.kwargs["selected"][-1] > hi for c in mid)
    assert any(len(np.unique(c.kwargs["selected"])) < len(c.kwargs["selected"]) for c in cases)
    assert changed >= len(cases) // 2
