"""The scenes of tests/test_gpu_odd_rings.py: rings whose x extent is no multiple of 16, of 4 or of anything, down to rows
of one voxel, filled whole from seeded numpy arrays (no SceneSpec, no chunk loader), and the windows and boxes set on
them.  Everything here is numpy and plain Python: the expected window of a LOD is cut from the SOURCE arrays, never from
a read-back, so that what the twins are given has not passed through the code under test.  tests/test_odd_ring_scenes.py
holds this module to what it claims (which row starts a window visits, that it wraps, that the x run crosses the seam).

Axis order: rings, offsets, shapes and boxes are (x, y, z), as in include/svr.h; arrays are numpy order [z][y][x]."""
import functools

import numpy as np

f32, U32 = np.float32, np.uint32

# name -> ring extents (x, y, z); what the row pitch does to the row starts is in the comments
RINGS = {
    "odd3": (63, 15, 25),      # x = 3 (mod 4): rows start 1 element apart (mod 4 and mod 16)
    "odd1": (21, 7, 9),        # x = 1 (mod 4)
    "even2": (42, 12, 10),     # x = 2 (mod 4): 2 apart
    "quad": (36, 6, 5),        # 4 divides x, 16 does not: 4 apart in a u8 or u16 slot
    "oct": (40, 5, 6),         # 8 divides x, 16 does not: 8 apart in a u8 slot
    "thin3": (3, 5, 7),        # rows shorter than a unit of 4
    "thin1": (1, 4, 6),        # rows of one voxel
}
DTYPE = {"uint8": np.uint8, "uint16": np.uint16, "float32": f32}
PER_SLOT = {"uint8": 16, "uint16": 8, "float32": 4}                   # elements of a 16-byte slot of the density ring
LEVEL = {"uint8": 128.0, "uint16": 128.0 * 251.0, "float32": 27.36}   # about half the voxels reach it
SELECTED = [1, 2, 3, 0xFFFFFFF0, 77]                                  # the seam objects, and an id nobody has
RUN_LABEL = 2

# key -> (geometry per LOD, density storage, label rings)
SCENES = {
    "odd3-u8": (["odd3"], "uint8", True),
    "odd3-u16": (["odd3"], "uint16", True),
    "odd3-f32": (["odd3"], "float32", True),
    "odd3-nolabels": (["odd3"], "uint8", False),
    "odd1-f32": (["odd1"], "float32", True),
    "even2-u16": (["even2"], "uint16", True),
    "quad-u8": (["quad"], "uint8", True),
    "oct-u8": (["oct"], "uint8", True),
    "thin3-u8": (["thin3"], "uint8", True),
    "thin1-u8": (["thin1"], "uint8", True),
    "odd3+odd1-u8": (["odd3", "odd1"], "uint8", True),                # LOD 1 begins behind an odd number of voxels
}
FAR_GEOMETRIES = ("odd3", "even2")
BOX_SCENES = ("odd3-u8", "odd3-f32")


def run_of(ring_x):
    """(length, before, behind) of the x run of RUN_LABEL: ring slots [ring_x - before, ring_x) and [0, behind)."""
    length = RUN_LENGTH.get(ring_x, 0)
    return length, length // 2, length - length // 2


# ring x -> voxels of the run: 40 where the ring is that wide, else what leaves a window room to begin beside it
RUN_LENGTH = {63: 40, 21: 12, 42: 24, 36: 27, 40: 31}


def slots_covered(spr):
    """The slots of a row that the lanes sharing it visit when the plan says ``spr`` (csrc/ring_pieces.h: a power of two
    of lanes up to 8, beyond that passes of 8 or more lanes): more than spr, which hides a plan that is one slot short
    unless spr sits on such a boundary."""
    if spr <= 8:
        return 1 << max(spr - 1, 0).bit_length()
    return -(-spr // 8) * 8


def last_slot_matters(ring_x, s, n, per_slot):
    """Whether a piece of rows of n voxels at x slot s of a full-height window has a row whose last voxels lie in a slot
    that the lanes would not visit had the plan counted the slots of the piece's first row alone: the rows begin
    (s + k ring_x) % per_slot elements into a slot, k counting the ring's rows."""
    worst = max(((s + k * ring_x) % per_slot + n + per_slot - 1) // per_slot for k in range(per_slot))
    return worst > slots_covered((s % per_slot + n + per_slot - 1) // per_slot)


def x_slot_score(ring_x, s, nx):
    """For how many of the slot sizes 4, 8 and 16 a window of nx voxels along x that begins at x slot s has such a piece."""
    first = min(nx, ring_x - s)
    pieces = [(s, first)] + ([(0, nx - first)] if first < nx else [])
    return sum(any(last_slot_matters(ring_x, ps, pn, per) for ps, pn in pieces) for per in (4, 8, 16))


def content(geometry, storage, seed):
    """(density, labels) of one whole ring, [z][y][x]: noise of which half reaches LEVEL (NaN and both infinities planted
    on float32); a dense background of labels {0, 9, 10}, a box of label 1 around the corner where the three wrap seams
    meet, boxes of 3 and 0xFFFFFFF0 across the y and the z seam, and one row of RUN_LABEL across the x seam."""
    rx, ry, rz = RINGS[geometry]
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (rz, ry, rx)).astype(np.uint8)
    lab = np.array([0, 9, 10], U32)[rng.integers(0, 3, (rz, ry, rx))]

    def put(xs, ys, zs, value):                                         # half-open ring slots, negative ones wrap
        lab[np.ix_(np.arange(*zs) % rz, np.arange(*ys) % ry, np.arange(*xs) % rx)] = value

    put((-2, 2), (-2, 2), (-2, 2), 1)
    put((5, 9), (-2, 2), (3, 5), 3)
    put((10, 14), (3, 5), (-2, 2), 0xFFFFFFF0)
    length, before, behind = run_of(rx)
    if length:
        put((-before, behind), (1, 2), (0, 1), RUN_LABEL)
    if storage == "uint16":
        d = d.astype(np.uint16) * np.uint16(251)
    if storage == "float32":
        d = d.astype(f32) * f32(0.37) - f32(20.0)
        k = max(3, d.size // 60)
        at = rng.choice(d.size, 3 * k, replace=False)
        flat = d.reshape(-1)
        flat[at[:k]], flat[at[k:2 * k]], flat[at[2 * k:]] = np.nan, np.inf, -np.inf
    return d, lab


class Lod:
    def __init__(self, geometry, storage, labels, seed):
        self.geometry, self.ring = geometry, RINGS[geometry]
        self.density, lab = content(geometry, storage, seed)
        self.labels = lab if labels else None

    def window(self, off, shape):
        """(off, shape, ring in numpy order, density f32, labels u32 or None) of the window, cut from the source arrays:
        the tuple the ``hold`` helpers of the components, distance and mesh tests take as ``window``."""
        idx = np.ix_(*[(int(off[a]) + np.arange(shape[a])) % self.ring[a] for a in (2, 1, 0)])
        return (list(off), list(shape), self.ring[::-1], self.density[idx].astype(f32), None if self.labels is None else self.labels[idx])

    def ring_dict(self, off, shape):
        """What histogram_twin and objects_twin take in place of a ring of ``oracle.lmip.rings_of``."""
        return dict(offset=tuple(off), shape=tuple(shape), density=self.density, labels=self.labels)


    def tails_range(self):
        """(lo, hi) with values of the ring below lo and above hi, and hi itself a value of the ring."""
        real = np.unique(self.density[np.isfinite(self.density)]).astype(f32)
        lo, hi = float(real[real.size // 4]) + 0.25, float(real[3 * real.size // 4])
        assert real.size >= 16 and (real < lo).any() and (real > hi).any() and lo < hi
        return lo, hi


def selections(has_labels):
    """The ``selected`` lists of a scene: the seam objects with a third of the background; without label rings every
    label reads 0, so a list passes everything or nothing."""
    return [SELECTED + [9]] if has_labels else [[0, 9], [5]]


class Scene:
    def __init__(self, key):
        geometries, self.storage, self.has_labels = SCENES[key]
        self.key = key
        self.lods = [Lod(g, self.storage, self.has_labels, 100 * list(SCENES).index(key) + k) for k, g in enumerate(geometries)]


_SCENES = {}


def scene(key):
    """Built once and left unchanged."""
    if key not in _SCENES:
        _SCENES[key] = Scene(key)
    return _SCENES[key]


def x_slots(ring_x, nx):
    """The ring slots at which a window of nx voxels along x may begin so that it holds the whole x run (any, without one)."""
    length, before, behind = run_of(ring_x)
    if not length:
        return list(range(ring_x))
    return [s for s in range(ring_x) if s <= ring_x - before and s + nx >= ring_x + behind]


@functools.lru_cache(maxsize=None)
def windows(geometry):
    """[(name, offset, shape)].  W-full: the whole ring's worth at four offsets whose x is 0, 1, 2, 3 (mod 4), beginning
    inside the ring on every axis that has an inside.  W-part: ring - (5, 2, 3), at least 1, beginning at the ring's last
    slot on y and z and so that the x run lies inside on x: it wraps wherever it is wider than one voxel.  W-far (two
    geometries): the W-part shape at 2^31 - 1 - shape, the last offset at which offset + shape still fits int32.
    Among the x slots these rules leave, the one is taken whose rows need their last slot on the most slot sizes
    (x_slot_score), then one no window has yet."""
    rx, ry, rz = ring = RINGS[geometry]
    out, used = [], set()
    slots = [s for s in x_slots(rx, rx) if s or rx == 1]
    for k in range(4):
        ox = max((o for o in range(2 * rx, 6 * rx + 4) if o % 4 == k and o % rx in slots),
                 key=lambda o: (x_slot_score(rx, o % rx, rx), o % rx not in used, -o))
        used.add(ox % rx)
        oy = ry * (k + 1) + 1 + (2 * k) % (ry - 1)
        oz = rz * (4 - k) + 1 + (3 * k) % (rz - 1)
        out.append((f"full{k}", (ox, oy, oz), ring))
    part = tuple(max(r - c, 1) for r, c in zip(ring, (5, 2, 3)))
    # an odd slot, so that x = 2 (mod 4) visits every row start, and not the last one, so that the run lies inside
    slots = [s for s in x_slots(rx, part[0])[:-1] if s % 2 and s + part[0] > rx]
    sx = rx - 1 if part[0] == 1 else max(slots, key=lambda s: (x_slot_score(rx, s, part[0]), s))
    out.append(("part", (3 * rx + sx, 2 * ry + ry - 1, rz + rz - 1), part))
    if geometry in FAR_GEOMETRIES:
        out.append(("far", tuple(2 ** 31 - 1 - n for n in part), part))
    return out


def pieces_of(ring, off, shape):
    """The window cut at the ring's wrap seams, as csrc/ring_pieces.h states it: [((sx, sy, sz), (nx, ny, nz))]."""
    runs = []
    for a in range(3):
        s0 = int(off[a]) % ring[a]
        first = min(shape[a], ring[a] - s0)
        runs.append([(s0, first)] + ([(0, shape[a] - first)] if first < shape[a] else []))
    return [((sx, sy, sz), (nx, ny, nz)) for sz, nz in runs[2] for sy, ny in runs[1] for sx, nx in runs[0]]


def row_starts(ring, off, shape, modulus):
    """[set of (element index of a row's first voxel) % modulus, per piece]: the ring's rows one by one."""
    out = []
    for (sx, sy, sz), (nx, ny, nz) in pieces_of(ring, off, shape):
        out.append({(((sz + z) * ring[1] + sy + y) * ring[0] + sx) % modulus for z in range(nz) for y in range(ny)})
    return out


def wraps(ring, off, shape):
    return tuple(int(off[a]) % ring[a] + shape[a] > ring[a] for a in range(3))


def longest_x_run(labels, value):
    """(length, first x) of the longest run of ``value`` along x in a [z][y][x] array."""
    best = (0, 0)
    for z, y in zip(*np.nonzero((labels == value).any(axis=2))):
        row = np.concatenate(([0], (labels[z, y] == value).astype(np.int8), [0]))
        edges = np.flatnonzero(np.diff(row))
        for b, e in zip(edges[::2], edges[1::2]):
            best = max(best, (int(e - b), int(b)))
    return best


def boxes(off, shape, ring):
    """[(name, (offset, shape))] on a W-part window of odd3: the whole window (None); rows of 1, 3, 4, 5 and 33 voxels
    along x at starts 0 .. 3 and at the two starts just before the x seam, across the y and the z seam; a box one voxel
    thick on each axis; one partly outside."""
    ox, oy, oz = off
    seam = ring[0] - ox % ring[0]                                      # the window's x at which the ring wraps
    assert 3 < seam - 2 and seam - 1 + 33 <= shape[0]
    out = [("window", None)]
    for nx in (1, 3, 4, 5, 33):
        for start in (0, 1, 2, 3, seam - 2, seam - 1):
            out.append((f"row {nx} at {start}", ((ox + start, oy, oz), (nx, 4, 5))))
    out += [("thin x", ((ox + 9, oy + 2, oz), (1, 9, 11))), ("thin y", ((ox + 9, oy + 2, oz), (41, 1, 11))),
            ("thin z", ((ox + 9, oy, oz + 1), (41, 9, 1))),
            ("partly outside", ((ox - 5, oy + 2, oz + shape[2] - 6), (20, shape[1] + 9, 30)))]
    return out


def plan_cases():
    """[(ring, window offset, lo, n)] of every window of every geometry, and of every box cut at its window: what the
    plans of the five passes are asked for by tests/test_gpu_odd_rings.py."""
    out = []
    for geometry, ring in RINGS.items():
        for name, off, shape in windows(geometry):
            out.append((ring, off, off, shape))
            if geometry == "odd3" and name == "part":
                for _, box in boxes(off, shape, ring)[1:]:
                    lo = tuple(max(off[a], box[0][a]) for a in range(3))
                    hi = tuple(min(off[a] + shape[a], box[0][a] + box[1][a]) for a in range(3))
                    out.append((ring, off, lo, tuple(h - l for l, h in zip(lo, hi))))
    return out
