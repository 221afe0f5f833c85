"""Input families for svr_outline at its edges, shared by the CPU tier (tests/test_outline.py holds the restatement
`outline_reference` to answers that do not come from it) and the GPU tier (tests/test_gpu_outline_edges.py holds the
kernel to the restatement bit for bit).  Every family yields `Case`s: the four planes of a frame as numpy arrays, the
keyword arguments of `outline_reference`, and a closed-form edge mask where one exists.  Closed forms are index
arithmetic on the one changed pixel, never `window_differs`.

The kernel (csrc/compose_kernels.hip) is not the brute-force window: 32 x 8 tiles with a border-replicated halo, a
separable row / column pass of label min / max from the neutral starts 0xFFFFFFFF / 0, a non-hit bit, depth min / max
through fminf / fmaxf with NaN staged for non-hits.  The families aim at those arguments: pixels on tile seams and
image corners, frames smaller than a tile or the halo, labels 0 and 0xFFFFFFFF, depths that are infinite, NaN or
signed zeros, a depth step of exactly the tolerance, flag bytes outside 0 .. 2."""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
U32 = np.uint32
HIT, MISS, DISCARD = 2, 1, 0
TOP = 0xFFFFFFFF
TILE_W, TILE_H = 32, 8                     # kOutlineTileW, kOutlineTileH
SUBNORMAL = F32(1e-41)
COLOR = (0.9, 0.2, 0.1, 0.8)


@dataclass
class Case:
    name: str
    rgba: np.ndarray                       # f32 [h, w, 4]
    depth: np.ndarray                      # f32 [h, w]
    label: np.ndarray                      # u32 [h, w]
    flags: np.ndarray                      # u8 [h, w]
    kwargs: dict                           # of outline_reference: radius, depth_tolerance, color, ...
    mask: np.ndarray = None                # closed-form edge mask, where one exists
    direct: bool = False                   # must go through the C entry point (Python's checks refuse or rewrite it)
    family: str = ""

    def __post_init__(self):
        h, w = self.flags.shape
        assert self.rgba.shape == (h, w, 4) and self.rgba.dtype == F32
        assert self.depth.shape == (h, w) and self.depth.dtype == F32
        assert self.label.shape == (h, w) and self.label.dtype == U32 and self.flags.dtype == np.uint8
        fl = np.unique(self.flags)
        tau = self.kwargs.get("depth_tolerance")
        if fl.max(initial=0) > 2 or (tau is not None and tau == 0 and np.signbit(tau)):
            self.direct = True


def reference(case, near=None):
    """(out, mask) of the restatement for one case."""
    from test_outline import outline_reference
    with np.errstate(all="ignore"):                                     # NaN and inf planes are inputs here
        return outline_reference(case.rgba, case.label, case.flags, depth=case.depth, near=near, **case.kwargs)


def random_rgba(shape, seed):
    return np.random.default_rng(seed).random((*shape, 4), dtype=F32)


def ball(h, w, y, x, r, centre):
    """Chebyshev ball of radius r round (y, x), clipped to the image, with or without its centre."""
    m = np.zeros((h, w), np.uint8)
    m[max(0, y - r):min(h, y + r + 1), max(0, x - r):min(w, x + r + 1)] = 1
    m[y, x] = 1 if centre else 0
    return m


# ---- family 1: one odd pixel in a uniform frame ----------------------------------------------------------------------
LONE_KINDS = {                              # kind -> (field label, odd label, odd flag byte)
    "larger": (5, 9, HIT), "smaller": (5, 2, HIT), "zero_in_top": (TOP, 0, HIT), "top_in_zero": (0, TOP, HIT),
    "miss": (5, 5, MISS), "discard": (5, 5, DISCARD), "flag3": (5, 5, 3), "flag255": (5, 5, 255),
}
LONE_FRAMES = [(70, 41, 1), (70, 41, 2), (70, 41, 7), (150, 90, 16)]        # w, h, r


def lone_positions(w, h):
    """(y, x): centre, the four image corners, either side of the first tile seam in x, in y, and in both."""
    cy, cx = h // 2, w // 2
    seam_x, seam_y = (TILE_W - 1, TILE_W), (TILE_H - 1, TILE_H)
    pos = [(cy, cx), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pos += [(cy, x) for x in seam_x] + [(y, cx) for y in seam_y] + [(y, x) for y in seam_y for x in seam_x]
    return pos


def lone_pixel_cases(kinds=None, frames=None):
    for w, h, r in frames or LONE_FRAMES:
        rgba = random_rgba((h, w), 3)
        for kind in kinds or LONE_KINDS:
            field_label, odd_label, odd_flag = LONE_KINDS[kind]
            for y, x in lone_positions(w, h):
                label = np.full((h, w), field_label, U32)
                flags = np.full((h, w), HIT, np.uint8)
                depth = np.full((h, w), 0.5, F32)
                label[y, x], flags[y, x] = odd_label, odd_flag
                yield Case(f"lone-{kind}-{w}x{h}-r{r}-y{y}x{x}", rgba, depth, label, flags,
                           dict(radius=r, depth_tolerance=0.0, color=COLOR), mask=ball(h, w, y, x, r, odd_flag == HIT),
                           family="lone")


# ---- family 5 (and 2): random blocky frames --------------------------------------------------------------------------
BLOCKY_IDS = (0, TOP, 7, 0x80000001, 300)
BLOCKY_FRAMES = [(70, 41, 1), (70, 41, 2), (70, 41, 7), (97, 61, 1), (97, 61, 2), (97, 61, 7), (150, 90, 16)]
TINY_FRAMES = [(1, 1), (1, 40), (40, 1), (5, 3), (31, 7), (32, 8), (33, 9), (64, 16)]       # w, h
TINY_RADII = (1, 7, 16)
PALETTE7 = np.array([(0.05, 0.5), (0.2, 1.0), (0.4, 0.25), (0.55, 0.75), (0.7, 0.5), (0.9, 1.0), (0.3, 0.0)], F32)


def palette(hs):
    hs = np.asarray(hs, F32).reshape(-1, 2)
    return np.concatenate([hs, np.full((len(hs), 1), 0.8, F32), np.ones((len(hs), 1), F32)], 1)


def blocky_planes(w, h, r, seed, ids=BLOCKY_IDS, quiet=True):
    """(rgba, depth, label, flags, tau).  3 to 5 axis-aligned label rectangles with sides >= 2r + 8 where the frame
    allows, over a background id; non-hit blobs with flag bytes 0, 1 and 3 over about 15 % of the frame, all of them in
    its left half, so that on the right the labels and the depths decide; a depth level
    per rectangle plus small noise on about half of the 8 x 8 cells.  The last rectangle is painted after the blobs
    and the noise: all hits, one label, one depth, so the pixels further than r from its border are non-edges whatever
    the depth test (the census of test_outline.py; `quiet` off for frames it would cover whole).  tau: the 0.9 quantile
    of the depth steps between horizontally adjacent hits of one label, as tests/test_gpu_outline.py takes it."""
    rng = np.random.default_rng(seed)
    side = 2 * r + 8
    label = np.full((h, w), ids[0], U32)
    depth = np.full((h, w), 0.25, F32)
    flags = np.full((h, w), HIT, np.uint8)
    k = int(rng.integers(3, 6))
    rects = []
    for i in range(k):
        rw, rh = min(w, side + int(rng.integers(0, 9))), min(h, side + int(rng.integers(0, 9)))
        x0, y0 = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
        rects.append((y0, x0, rh, rw, ids[(i + 1) % len(ids)], F32(0.3 + 0.1 * i)))
    for y0, x0, rh, rw, lid, z in rects[:-1]:
        label[y0:y0 + rh, x0:x0 + rw], depth[y0:y0 + rh, x0:x0 + rw] = lid, z
    cells = rng.random((-(-h // 8), -(-w // 8))) < 0.5
    noisy = np.repeat(np.repeat(cells, 8, 0), 8, 1)[:h, :w]
    depth = (depth + np.where(noisy, rng.random((h, w), dtype=F32) * F32(1e-3), F32(0))).astype(F32)
    while np.count_nonzero(flags != HIT) < 0.15 * w * h:
        bh, bw = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, max(1, int(0.45 * w))))
        flags[y0:y0 + bh, x0:x0 + bw] = rng.choice([DISCARD, MISS, 3])
    if quiet:
        y0, x0, rh, rw, lid, z = rects[-1]
        label[y0:y0 + rh, x0:x0 + rw], depth[y0:y0 + rh, x0:x0 + rw], flags[y0:y0 + rh, x0:x0 + rw] = lid, z, HIT
    rgba = random_rgba((h, w), seed + 1000)
    rgba[flags == MISS] = (0, 0, 0, 1)
    rgba[flags == DISCARD] = 0
    hit = flags == HIT
    pair = hit[:, 1:] & hit[:, :-1] & (label[:, 1:] == label[:, :-1])
    steps = np.abs(depth[:, 1:] - depth[:, :-1])[pair]
    tau = float(np.quantile(steps, 0.9)) if steps.size else 0.0
    return rgba, depth, label, flags, tau


def blocky_variants():
    """The keyword sets every blocky frame runs with (the window test is shared: one `near` per frame, r and tau)."""
    return [dict(color=COLOR),
            dict(color=COLOR, color_by_label=True, colors=palette(PALETTE7), selected=[0, TOP], dim_unselected=0.25),
            dict(color=(0.1, 0.3, 0.7, 1.0), selected=[7, 300, TOP], dim_unselected=0.5, only_selected=True)]


def blocky_frames(frames=None):
    """(name, planes, r, tau or None) per frame, radius and depth test on / off."""
    for w, h, r in frames or BLOCKY_FRAMES:
        planes = blocky_planes(w, h, r, seed=40 + BLOCKY_FRAMES.index((w, h, r)))      # a frame is the same whoever asks
        for z_on in (False, True):
            yield f"blocky-{w}x{h}-r{r}-{'z_on' if z_on else 'z_off'}", planes, r, (planes[4] if z_on else None)


def tiny_frames():
    for n, (w, h) in enumerate(TINY_FRAMES):
        for r in ((16,) if (w, h) == (5, 3) else TINY_RADII):
            planes = blocky_planes(w, h, r, seed=80 + n, quiet=False)
            for z_on in (False, True):
                yield f"tiny-{w}x{h}-r{r}-{'z_on' if z_on else 'z_off'}", planes, r, (planes[4] if z_on else None)


def cases_of_frame(name, planes, r, tau, family):
    rgba, depth, label, flags, _ = planes
    for i, kw in enumerate(blocky_variants()):
        yield Case(f"{name}-v{i}", rgba, depth, label, flags, dict(radius=r, depth_tolerance=tau, **kw), family=family)


# ---- family 3: depth -------------------------------------------------------------------------------------------------
DEPTH_FRAME = (70, 41)                      # w, h: the odd pixel sits across the first tile seam in x
DEPTH_ODD = (20, 33)                        # y, x
DEPTH_RADII = (1, 2, 16)
DEPTH_SPECIALS = {"+inf": F32(np.inf), "-inf": F32(-np.inf), "nan": F32(np.nan), "-0": F32(-0.0), "+0": F32(0.0),
                  "subnormal": SUBNORMAL}
DEPTH_TAUS = {"0": F32(0.0), "-0": F32(-0.0), "+inf": F32(np.inf), "1e-3": F32(1e-3)}


def depth_frame(field_z, odd_z, r, tau, name, mask, odd_flag=HIT):
    w, h = DEPTH_FRAME
    y, x = DEPTH_ODD
    depth = np.full((h, w), field_z, F32)
    depth[y, x] = odd_z
    flags = np.full((h, w), HIT, np.uint8)
    flags[y, x] = odd_flag
    return Case(name, random_rgba((h, w), 5), depth, np.full((h, w), 11, U32), flags,
                dict(radius=r, depth_tolerance=tau, color=COLOR), mask=mask, family="depth")


def strict_step_values():
    """(field, tau, {name: (odd depth, edge?)}): odd pixels whose f32 difference from the field is exactly tau (no edge:
    the test is strict) and exactly nextafter(tau, inf) (edge), above and below the field.  0.0625 and 0.125 make every
    one of those sums exact in f32, which the float64 asserts prove."""
    z0, tau = F32(0.0625), F32(0.125)
    up = np.nextafter(tau, F32(np.inf))
    odd = {"above_by_tau": (F32(z0 + tau), False), "above_by_next": (F32(z0 + up), True),
           "below_by_tau": (F32(z0 - tau), False), "below_by_next": (F32(z0 - up), True)}
    for name, (z, edge) in odd.items():
        d = abs(float(z) - float(z0))
        assert d == (float(up) if edge else float(tau)) and F32(d) == F32(abs(z - z0)), name
    return z0, tau, odd


def depth_cases(radii=DEPTH_RADII):
    """r = 16 runs the table of special values under two of the four tolerances: the other two repeat its edges at a
    window of 33 x 33, the costly one for the restatement."""
    w, h = DEPTH_FRAME
    y, x = DEPTH_ODD
    z0, tau, odd = strict_step_values()
    for r in radii:
        for name, (z, edge) in odd.items():
            mask = ball(h, w, y, x, r, True) if edge else np.zeros((h, w), np.uint8)
            yield depth_frame(z0, z, r, float(tau), f"depth-{name}-r{r}", mask)
        for fname, fz in DEPTH_SPECIALS.items():
            for oname, oz in DEPTH_SPECIALS.items():
                for tname, t in DEPTH_TAUS.items():
                    if r == 16 and tname not in ("-0", "1e-3"):
                        continue
                    with np.errstate(invalid="ignore"):
                        differs = bool(np.abs(F32(oz - fz)) > t)             # NaN on either side: False
                    mask = ball(h, w, y, x, r, True) if differs else np.zeros((h, w), np.uint8)
                    yield depth_frame(fz, oz, r, float(t), f"depth-field{fname}-odd{oname}-tau{tname}-r{r}", mask)
        # a non-hit keeps a stale depth far from the field: a silhouette edge round it and nothing else
        for flag in (MISS, DISCARD):
            yield depth_frame(F32(0.5), F32(1e30), r, 0.1, f"depth-stale-flag{flag}-r{r}", ball(h, w, y, x, r, False), flag)


# ---- hand-made frames with written-out answers -----------------------------------------------------------------------
def row_case(name, labels, depths, r, tau, mask):
    n = len(labels)
    return Case(name, random_rgba((1, n), 9), np.array([depths], F32), np.array([labels], U32),
                np.full((1, n), HIT, np.uint8), dict(radius=r, depth_tolerance=tau, color=COLOR),
                mask=np.array([mask], np.uint8), family="hand")


def hand_cases():
    inf, nan = np.inf, np.nan
    yield row_case("hand-1x1-r16", [3], [0.5], 16, 0.0, [0])
    yield row_case("hand-top-labels-inf-nan", [0, TOP, TOP], [inf, inf, nan], 1, 0.0, [1, 1, 0])
    yield row_case("hand-inf-minus-inf", [4, 4, 4], [inf, inf, -inf], 1, 1e30, [0, 1, 1])
    yield row_case("hand-nan-between-r1", [4, 4, 4], [0.5, nan, 0.75], 1, 0.1, [0, 0, 0])
    yield row_case("hand-nan-between-r2", [4, 4, 4], [0.5, nan, 0.75], 2, 0.1, [1, 0, 1])


# ---- family 4: colour ------------------------------------------------------------------------------------------------
HUES = [0.0, float(np.nextafter(F32(1 / 6), F32(0))), float(F32(1 / 6)), float(np.nextafter(F32(1 / 6), F32(1))),
        0.999999, 1.0, 1.25, -0.1, 1e30, float("nan")]
SATURATIONS = [0.0, 0.5, 1.0]
MODULO_LABELS = [TOP, 0x80000000, 0, 5, 0x7FFFFFFF, 0xFFFFFFFE, 0x80000001, 6]
RGBA_SPECIALS = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0, 1e-41, -1e-41, 1e-38, 3.4e38, 0.25], F32)


def striped(labels, h=2, seed=13, flags=None):
    """One column per label: at r = 1 every hit with a neighbour column is an edge."""
    lab = np.repeat(np.array([labels], U32), h, 0)
    fl = np.full(lab.shape, HIT, np.uint8) if flags is None else flags
    return random_rgba(lab.shape, seed), np.full(lab.shape, 0.5, F32), lab, fl


def color_cases():
    rng = np.random.default_rng(17)
    for count in (1, 3, 7):
        pal = palette(np.stack([rng.random(count, dtype=F32), rng.random(count, dtype=F32) * F32(0.9) + F32(0.1)], 1))
        yield Case(f"color-modulo-{count}", *striped(MODULO_LABELS),
                   dict(radius=1, color=(0, 0, 0, 1.0), color_by_label=True, colors=pal), family="color",
                   mask=np.ones((2, len(MODULO_LABELS)), np.uint8))
    pal = palette([(hh, s) for s in SATURATIONS for hh in HUES])
    n = len(pal)
    for a in (1.0, 0.6):
        yield Case(f"color-hues-a{a}", *striped(np.arange(n) + 3 * n), dict(radius=1, color=(0, 0, 0, a), color_by_label=True,
                                                                          colors=pal), family="color")
    for a in (0.0, 1.0):
        for by in (False, True):
            yield Case(f"color-opacity{a:g}-by{int(by)}", *striped([1, 2, 3, 4, 5, 6]),
                       dict(radius=1, color=(0.3, 0.6, 0.9, a), color_by_label=by, colors=palette(PALETTE7)), family="color")
    # dimming: subnormal RGBA times 0, 1 and 1e-3 (products that are subnormal or round to zero)
    for dim in (0.0, 1.0, 1e-3):
        rgba, depth, lab, fl = striped([1, 1, 1, 2, 2, 2, 2, 3, 3, 3], h=3)
        rgba = (rng.integers(1, 1 << 20, rgba.shape).astype(U32) | (rng.integers(0, 2, rgba.shape).astype(U32) << 31)).view(F32)
        yield Case(f"color-dim{dim:g}-subnormal", rgba, depth, lab, fl,
                   dict(radius=1, color=(0.3, 0.6, 0.9, 0.5), selected=[2], dim_unselected=dim), family="color")
    # special RGBA on hits, misses and discards, blended, dimmed and passed through
    lab = np.repeat(np.array([[1] * 6 + [2] * 6 + [3] * 6], U32), 6, 0)
    fl = np.full(lab.shape, HIT, np.uint8)
    fl[1, :], fl[4, ::2] = MISS, DISCARD
    rgba = rng.choice(RGBA_SPECIALS, (*lab.shape, 4)).astype(F32)
    for a in (0.0, 0.5, 1.0):
        yield Case(f"color-special-rgba-a{a:g}", rgba, np.full(lab.shape, 0.5, F32), lab, fl,
                   dict(radius=2, color=(0.3, 0.6, 0.9, a), selected=[1, 3], dim_unselected=0.5), family="color")


# ---- family 6: selections as the C entry point takes them ------------------------------------------------------------
MID_IDS = (100, 0xFFFFFF00, 7000, 0x80000001, 300)


def selection_cases():
    """Sorted id arrays handed over as they are (`selected` is a numpy u32 array: the GPU tier passes it on untouched;
    the restatement de-duplicates it, which changes no membership)."""
    rng = np.random.default_rng(23)
    w, h, r = 70, 41, 2
    many = np.sort(np.concatenate([rng.integers(0, 1 << 32, 995, dtype=np.uint64), [0, 7, 300, 300, TOP]])).astype(U32)
    frames = {
        "ends": (blocky_planes(w, h, r, 61, BLOCKY_IDS),
                 [[0], [TOP], [5], [0, TOP], [7, TOP], [0, 7, TOP], [0, 300, 0x80000001], [0, 0, 7, 7, 7, TOP, TOP], many]),
        "mid": (blocky_planes(w, h, r, 62, MID_IDS),
                [[5], [0xFFFFFFF0], [5, 0xFFFFFFF0], [5, 300, 0xFFFFFFF0], [0, 100, TOP], [100, 100, 300, 300, 7000]]),
    }
    for fname, (planes, sels) in frames.items():
        rgba, depth, label, flags, tau = planes
        for i, sel in enumerate(sels):
            sel = np.asarray(sel, U32)
            assert np.all(sel[1:] >= sel[:-1])
            for only in (False, True):
                yield Case(f"selection-{fname}-{i}-n{len(sel)}-only{int(only)}", rgba, depth, label, flags,
                           dict(radius=r, depth_tolerance=tau, color=COLOR, selected=sel, dim_unselected=0.25,
                                only_selected=only), direct=True, family="selection")


def frame_cases(frames, family):
    """[(frame name, planes, r, tau, [cases])]: the cases of one frame share its window test."""
    return [(name, planes, r, tau, list(cases_of_frame(name, planes, r, tau, family))) for name, planes, r, tau in frames]
