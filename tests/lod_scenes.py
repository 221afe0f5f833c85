"""Scenes with 1 .. 8 LODs in which every LOD is the one that resolves a sample somewhere, shared by
tests/test_lod_counts.py (the conditions, on the numpy twins) and tests/test_gpu_lod_counts.py (the kernels).

Asking the usual cubic scene builders for more LODs does not reach the coarse slots: from LOD 3 on every window covers
the whole volume, so the first of them wins everywhere.  Here the volume is long and thin — 32 x 64 x 1024 voxels
(z, y, x), or 40 x 48 x 1152 for extents that are no powers of two — and the levels are downsampled per axis: x halves
at every level (scale down to 2^-7), y and z stop at a floor of a few voxels.  The window of LOD l spans a growing share
of every axis (1/8 .. 3/4 of x), so the windows are nested shells around the focus and LOD l alone holds the shell
between window l - 1 and window l; outside the last window no LOD holds a point.  The world transform squeezes x so that
the volume is about 64 x 64 x 32 world units: a 48 x 40 frame sees every shell, and rays that look mostly along z stay
short in data space.  The focus is off the chunk grids, so windows wrap their rings on every axis.

The densities are integer closed forms per level (sparse bright blobs on a dark, noisy background, a different phase
per level: a sample taken from the wrong level shows) plus, for every LOD l >= 1, bright voxels of level l just
outside window l - 1 on both sides along x: the first thing a ray meets when it leaves the finer window, in a stretch
whose index box the finer window holds only in part."""
import functools

import numpy as np

from oracle import ring_oracle
from sub_volume_renderer_amd import testing

MAX_LODS = 8
WIDTH, HEIGHT = 48, 40
STORAGES = ("u8", "u16", "f32")
KINDS = {"pow2": (32, 64, 1024), "odd": (40, 48, 1152)}          # base shape (z, y, x)
_FLOOR = {"pow2": (8, 8, 8), "odd": (5, 6, 9)}                    # the smallest extent a coarse level shrinks to
# the share of each axis (z, y, x) the window of LOD l asks for
_SHARE = [(1 / 2, 3 / 8, 1 / 8), (5 / 8, 1 / 2, 3 / 16), (3 / 4, 5 / 8, 1 / 4), (3 / 4, 3 / 4, 5 / 16),
          (7 / 8, 7 / 8, 3 / 8), (1, 1, 1 / 2), (1, 1, 5 / 8), (1, 1, 3 / 4)]
_FOCUS_OFF = (1.4, -2.7, 21.3)                                    # focus - volume middle, data voxels (z, y, x)


def _pow2_floor(n):
    return 1 << (int(n).bit_length() - 1)


def _round_up(n, m):
    return -(-n // m) * m


@functools.lru_cache(maxsize=None)
def geometry(kind, mixed=False):
    """Per LOD: dict(shape, chunk, ring (in chunks), size (the window asked for), all (z, y, x)), plus the focus in data
    voxels (z, y, x).  ``mixed``: the y extent of the rings of the odd levels is no multiple of 8, so those levels get
    no macro-cell grid; every other ring extent is a multiple of 8."""
    base = KINDS[kind]
    levels = []
    for l in range(MAX_LODS):
        shape = tuple(max(b >> l, f) for b, f in zip(base, _FLOOR[kind]))
        assert all(b % s == 0 for b, s in zip(base, shape))
        size = tuple(max(2, min(s, int(round(f * s)))) for s, f in zip(shape, _SHARE[l]))
        chunk = tuple(min(16, _pow2_floor(max(1, w // 6))) for w in size)
        ring = []
        for a in range(3):
            c = chunk[a]
            need = min(size[a] + 2 * c, _round_up(shape[a], c))   # the snapped window never exceeds either
            r = _round_up(need, max(8, c))
            if mixed and l % 2 == 1 and a == 1:
                while r % 8 == 0:
                    r += c
            ring.append(r // c)
        levels.append(dict(shape=shape, chunk=chunk, ring=tuple(ring), size=size))
    focus = tuple(b / 2 + o for b, o in zip(base, _FOCUS_OFF))
    return levels, focus


def windows(kind, mixed=False):
    """The window (offset, shape) of every LOD in its own voxels (z, y, x) after the scene's one center_on_position:
    what SubVolume.center_on_position does, restated on oracle.ring_oracle's ROI helpers."""
    levels, focus = geometry(kind, mixed)
    base = KINDS[kind]
    out = []
    for L in levels:
        scale = [s / b for s, b in zip(L["shape"], base)]
        offset = tuple(int(c * f - s // 2) for c, f, s in zip(focus, scale, L["size"]))
        r = ring_oracle.roi_intersect(ring_oracle.roi(offset, L["size"]), ring_oracle.roi((0, 0, 0), L["shape"]))
        out.append(ring_oracle.roi_snap_grow(r, L["chunk"]))
    return out


def _tri(u, p):
    m = u % p
    return np.minimum(m, p - m) * 512 // p                        # 0 .. 256


def _hash(z, y, x, l):
    h = (z * 73856093) ^ (y * 19349663) ^ (x * 83492791) ^ (l * 2654435761)
    h &= 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0x5BD1E995) & 0xFFFFFFFF
    return h ^ (h >> 15)


@functools.lru_cache(maxsize=None)
def _pairs(kind):
    """(density uint8, labels uint32) of the eight levels; read-only."""
    levels, focus = geometry(kind)
    base = KINDS[kind]
    wins = windows(kind)
    out = []
    for l, L in enumerate(levels):
        sz, sy, sx = L["shape"]
        z, y, x = np.ogrid[:sz, :sy, :sx]
        z, y, x = z.astype(np.int64), y.astype(np.int64), x.astype(np.int64)
        pz, py, px = max(4, 16 >> l), max(5, 24 >> l), max(7, 40 >> l)
        prod = (_tri(x + 3 * l, px) * _tri(y + 5 * l + x // 7, py) * _tri(z + l + y // 5, pz)) >> 16       # 0 .. 256
        dens = np.clip(prod * 3 - 160, 0, 235) + (_hash(z, y, x, l) & 15)
        lab = 1 + ((x // 3) * 7 + (y // 2) * 3 + z + l) % 200
        lab = np.where(dens < 32, 0, lab)
        if l:
            # bright voxels of this level just outside the finer window along x, on the focus' row
            vox = base[2] // sx
            (o, s) = wins[l - 1]
            fine = base[2] // levels[l - 1]["shape"][2]
            lo, hi = o[2] * fine, (o[2] + s[2]) * fine                         # the finer window in data voxels
            iz, iy = int(focus[0] * sz / base[0]), int(focus[1] * sy / base[1])
            for ix in (hi // vox, -(-lo // vox) - 1):
                if 0 <= ix < sx:
                    dens[iz, iy, ix] = 255
                    lab[iz, iy, ix] = 200 + l
        d, s = dens.astype(np.uint8), lab.astype(np.uint32)
        d.setflags(write=False)
        s.setflags(write=False)
        out.append((d, s))
    return tuple(out)


def vmax(storage):
    return 65535.0 if storage == "u16" else 255.0


def scene(nl, storage="u8", kind="pow2", mixed=False):
    """The SceneSpec of the first ``nl`` levels.  ``storage``: "u8" byte rings, "u16" uint16 sources (x 257) and rings,
    "f32" the byte sources in float32 rings."""
    assert 1 <= nl <= MAX_LODS and storage in STORAGES
    levels, focus = geometry(kind, mixed)
    levels = levels[:nl]
    pairs = list(_pairs(kind)[:nl])
    if storage == "u16":
        pairs = [(d.astype(np.uint16) * np.uint16(257), s) for d, s in pairs]
    base = KINDS[kind]
    world_scale = (64.0 / base[2], 1.0, 1.0)                       # x squeezed to 64 world units
    centre = tuple(float(f * s) for f, s in zip(focus[::-1], world_scale))
    top = vmax(storage)
    spec = testing.SceneSpec(
        pairs=pairs, chunk_shapes=[L["chunk"] for L in levels], ring_shapes=[L["ring"] for L in levels],
        material=dict(lmip_threshold=0.5 * top, lmip_fall_off=0.5, lmip_max_samples=10, fog_density=0.01,
                      fog_color=(0.5, 0.5, 0.5), colors=[(k / 4, 1.0, 1.0) for k in range(4)], clim=(0.0, top)),
        width=WIDTH, height=HEIGHT, depth_range=(0.5, 500.0), world_scale=world_scale,
        centers=[(centre, [L["size"] for L in levels])])
    if storage == "f32":
        spec.ring_storage = "float32"
    return camera(spec, "top")


def focus_world(spec):
    return np.array(spec.centers[0][0], np.float64)


CAMERAS = ("top", "side")
ISO_LEVELS = (0.3, 0.6)          # iso values the tests render, as fractions of the value range


def camera(spec, name):
    """Point the spec's camera: "top" an orthographic view down z, tilted a little, that sees the whole x-y extent (every
    shell under some pixel; the off-centre rays pass through the coarse shells only); "side" a perspective view from
    a corner towards the focus."""
    f = focus_world(spec)
    if name == "top":
        spec.projection, spec.ortho_size = "orthographic", (70.0, 70.0 * HEIGHT / WIDTH)
        spec.cam_position, spec.cam_target = tuple(f + np.array([4.0, -6.0, 70.0])), tuple(f)
    else:
        assert name == "side", name
        spec.projection, spec.fov = "perspective", 50.0
        spec.cam_position, spec.cam_target = tuple(f + np.array([-30.0, 22.0, 48.0])), tuple(f + np.array([6.0, -3.0, 0.0]))
    return spec


def slice_planes(spec, pixel=1.45):
    """(name, origin, u, v) in world units: a z-normal plane and an oblique one through a point next to the focus, at a
    pixel size at which the frame spans every shell."""
    origin = tuple(focus_world(spec) + np.array([0.13, -0.21, 0.07]))
    return [("z", origin, (pixel, 0.0, 0.0), (0.0, pixel, 0.0)),
            ("oblique", origin, (0.96 * pixel, 0.28 * pixel, 0.0), (-0.12 * pixel, 0.7 * pixel, 0.7 * pixel))]


def slab_steps():
    """(w, samples) of the slabs: a skew world step, so that one pixel's samples cross shell borders."""
    return (0.31, -0.23, 0.41), 7


FLY = ((27.0, 36.5, 12.0), (38.5, 28.0, 19.5))                    # world positions of the fly-through moves


def wraps(orac):
    """offset % ring of every LOD, shader order."""
    return [tuple(int(o) % r for o, r in zip(b.uniform()["offset"], b.texture.shape[::-1])) for b in orac.wrapping_buffers]
