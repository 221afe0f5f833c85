"""svr_compose (include/svr.h) restated in float64, and the synthetic input families its tests share.

TEST INFRASTRUCTURE ONLY.  ``reference`` states the operations of the kernel in float64 on what the kernel sees: the
planes, the background, ``t = (y + 0.5) / h`` and every constant are first rounded to float32 (the comparisons of the
depth test are exact in any precision), then nothing is rounded again.  It returns the real-valued
``v = clamp(c) * 255 + 0.5`` of every channel *before* the floor, so that a test can tell a value the float32 kernel
must get right from one that lies on a level's threshold:

    a value is *decidable* when |v - rint(v)| > DELTA, DELTA = 1e-3 levels.

Why 1e-3: with ``powf`` within 2 ulp the kernel's v lies within about 255 * 1.055 * 2 * 2^-24 ~ 3e-5 of the float64
value, the roundings of the blend (two products, a sum, the encode's multiply and subtract, * 255 + 0.5) add a few
times that; DELTA is about 20 times the bound.  On a decidable value the kernel must give floor(v) exactly; on the
others it may be one level off.  DELTA is fixed by this reasoning, not by what a kernel gives.
"""
import numpy as np

f32, f64 = np.float32, np.float64
DELTA = 1e-3

KNEE = f32(0.0031308)
_LIN, _A, _B = f64(f32(12.92)), f64(f32(1.055)), f64(f32(0.055))
_EXP = f64(f32(1.0) / f32(2.4))                     # 1.0f / 2.4f, a float32 division


def clamp01(c):
    """fminf(fmaxf(c, 0), 1): NaN -> 0."""
    return np.fmin(np.fmax(c, 0.0), 1.0)


def srgb_encode(c):
    c = clamp01(np.asarray(c, f64))
    with np.errstate(invalid="ignore"):
        return np.where(c <= f64(KNEE), _LIN * c, _A * np.power(c, _EXP) - _B)


def reference(rgba, depth=None, flags=None, bg_bottom=(0, 0, 0, 1), bg_top=(0, 0, 0, 1), zbuf=None, srgb=True):
    """(v float64 [h, w, 4], draw bool [h, w]): the value of every channel before the floor, and which pixels blend."""
    rgba = np.asarray(rgba, f32)
    h, w = rgba.shape[:2]
    t = ((np.arange(h, dtype=f32) + f32(0.5)) / f32(h)).astype(f64)[:, None, None]
    top, bottom = np.asarray(bg_top, f32).astype(f64), np.asarray(bg_bottom, f32).astype(f64)
    c = np.broadcast_to(top[None, None, :] * (1.0 - t) + bottom[None, None, :] * t, (h, w, 4))
    draw = np.ones((h, w), bool) if flags is None else (np.asarray(flags) != 0)
    if zbuf is not None:
        with np.errstate(invalid="ignore"):
            draw = draw & (np.asarray(depth, f32) < np.asarray(zbuf, f32))
    s = rgba.astype(f64)
    a = s[..., 3:4]
    with np.errstate(invalid="ignore", over="ignore"):
        over = np.concatenate([s[..., :3] * a + c[..., :3] * (1.0 - a), a + c[..., 3:4] * (1.0 - a)], axis=-1)
        c = np.where(draw[..., None], over, c)
        if srgb:
            c = np.concatenate([srgb_encode(c[..., :3]), c[..., 3:4]], axis=-1)
        v = clamp01(c) * 255.0 + 0.5
    return v, draw


def decidable(v):
    return np.abs(v - np.rint(v)) > DELTA


def levels(v):
    return np.floor(v).astype(np.uint8)


def hold(got, v, what=""):
    """``got`` (uint8, shaped like v) against the reference: floor(v) on every decidable value, within one level on the
    rest.  Returns (undecidable values, how many of them are one level off)."""
    want = np.floor(v).astype(np.int16)
    diff = np.abs(np.asarray(got).astype(np.int16) - want)
    dec = decidable(v)
    bad = dec & (diff != 0)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), np.asarray(got)[bad][:4], v[bad][:4])
    assert diff.max(initial=0) <= 1, (what, int(diff.max()), v[diff > 1][:4])
    return int((~dec).sum()), int((~dec & (diff != 0)).sum())


# ---- the synthetic input families ---------------------------------------------------------------------------------
# Backgrounds lie off the k / 255 grid.  Every pixel of a row that shows the background has the same v, so in a frame
# of 61 rows one row whose background lands within DELTA of a level already makes > 1 % of a channel undecidable: the
# backgrounds and seeds below were chosen, from the float64 reference alone, so that no family has such a row
# (test_compose.py asserts the share).
BG_OPAQUE = ((0.3927, 0.3941, 0.3963, 1.0), (0.6611, 0.6547, 0.6583, 1.0))            # (bottom, top)
BG_TRANSLUCENT = ((0.3997, 0.4011, 0.4033, 0.5), (0.6611, 0.6547, 0.6583, 0.25))


def planes(seed, h, w):
    """rgba uniform in [0, 1) with a third of the pixels at alpha 0 or 1 and a band of rows (or, in a one-row frame,
    of columns) with rgb and alpha outside [0, 1]; flags 0 / 1 / 2; depth and zbuf uniform, with a quarter of the
    pixels at depth == zbuf bit for bit."""
    rng = np.random.default_rng(seed)
    rgba = rng.random((h, w, 4), dtype=f32)
    pick = rng.integers(0, 6, (h, w))
    rgba[..., 3][pick == 0] = 0.0
    rgba[..., 3][pick == 1] = 1.0
    band = rgba[h // 3:h // 3 + max(1, h // 8)] if h > 1 else rgba[:, w // 3:w // 3 + max(1, w // 8)]
    band[...] = band * f32(3.0) - f32(1.0)                              # [-1, 2)
    flags = rng.integers(0, 3, (h, w)).astype(np.uint8)
    depth = rng.random((h, w), dtype=f32)
    zbuf = rng.random((h, w), dtype=f32)
    same = rng.integers(0, 4, (h, w)) == 0
    zbuf[same] = depth[same]
    return dict(rgba=rgba, flags=flags, depth=depth, zbuf=zbuf)


# (name "w x h", seed, h, w, background); the GPU tests cross them with the plane combinations
FAMILIES = [
    ("1x1", 11, 1, 1, BG_OPAQUE),
    ("257x1", 12, 1, 257, BG_OPAQUE),
    ("1x257", 14, 257, 1, BG_TRANSLUCENT),
    ("97x61", 18, 61, 97, BG_OPAQUE),
    ("97x61_translucent", 19, 61, 97, BG_TRANSLUCENT),
    ("256x256", 15, 256, 256, BG_TRANSLUCENT),
    ("gradient_3x4096", 16, 4096, 3, BG_OPAQUE),
]
BIG = ("2048x1025", 17, 1025, 2048, BG_OPAQUE)
# (name, uses flags, uses zbuf, passes depth)
COMBOS = [
    ("noflags_nodepth", False, False, False),
    ("noflags_ztest", False, True, True),
    ("flags_ztest", True, True, True),
    ("flags_depth_without_zbuf", True, False, True),
]


def combo_args(p, combo):
    """The oracle's / reference's keyword planes of one combination."""
    _, use_flags, use_z, use_depth = combo
    return dict(depth=p["depth"] if use_depth else None, flags=p["flags"] if use_flags else None,
                zbuf=p["zbuf"] if use_z else None)
