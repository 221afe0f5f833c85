"""The scene of tests/test_gpu_components.py: a 64 x 64 x 128 volume (numpy order) behind a ring of 72 x 16 x 40 voxels
(LOD 1: every second voxel, ring 36 x 12 x 20) whose window, centred on CENTRE, wraps on all three axes: the seams lie at
x = 72, y = 32 and z = 40.  A dense background of small objects, objects across each seam and one across the corner where
the three seams meet, one label near 2^32, and planted structures whose components are known (PLANTED)."""
import numpy as np

from sub_volume_renderer_amd import testing

f32 = np.float32
CENTRE = (84.0, 30.0, 36.0)                                          # world = data position (x, y, z)
LEVEL = {"u8": 128.0, "u16": 128.0 * 251.0, "f32": 27.36}            # about half the voxels reach it
HIGH = {"u8": 250.0, "u16": 250.0 * 251.0, "f32": 250.0 * 0.37 - 20.0}      # only the planted structures and a few specks do
# a one-voxel path through these corners (x, y, z): it crosses the x seam, then the y seam, then the z seam, and comes back
PATH = [(60, 26, 34), (84, 26, 34), (84, 38, 34), (84, 38, 46), (88, 38, 46), (88, 26, 46), (88, 26, 36)]
CORNER_PAIR = [(71, 35, 50), (72, 36, 51)]                           # touch at a corner only, across the x seam
FACE_PAIR = [(100, 30, 30), (101, 30, 30)]                           # labels 6 and 7 face to face
CHECKER = ((100, 24, 18), (16, 8, 8))                                # a box (offset, shape) of label 8 on a checkerboard, label 0 between
PLANTED = {"path": 4, "corner": 5, "face": (6, 7), "checker": 8}


def path_voxels():
    out = [PATH[0]]
    for a, b in zip(PATH, PATH[1:]):
        axis = [k for k in range(3) if a[k] != b[k]]
        assert len(axis) == 1
        step = 1 if b[axis[0]] > a[axis[0]] else -1
        p = list(a)
        while tuple(p) != b:
            p[axis[0]] += step
            out.append(tuple(p))
    assert len(set(out)) == len(out)
    return out


def volumes(kind):
    """[(density, labels)] of LOD 0 (64 x 64 x 128, numpy order) and LOD 1 (every second voxel)."""
    z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(128), indexing="ij")
    rng = np.random.default_rng(7)
    d = ((3 * x + 5 * y + 2 * z + rng.integers(0, 90, x.shape)) % 256).astype(np.uint8)
    d[d >= 250] = 249                                                   # HIGH is for what is planted below, and the specks
    d[rng.random(x.shape) < 0.002] = 255
    lab = np.array([0, 9, 10], np.uint32)[rng.integers(0, 3, x.shape)]          # a dense background of small objects
    lab[(x - 72) ** 2 + (y - 32) ** 2 + (z - 40) ** 2 <= 25] = 1                # across the corner where the three seams meet
    lab[(x >= 68) & (x < 76) & (y >= 27) & (y < 30) & (z >= 22) & (z < 27)] = 2             # across the x seam (72)
    lab[(x >= 56) & (x < 60) & (y >= 29) & (y < 35) & (z >= 44) & (z < 50)] = 3             # across the y seam (32)
    lab[(x >= 90) & (x < 95) & (y >= 27) & (y < 31) & (z >= 36) & (z < 44)] = 0xFFFFFFF0    # across the z seam (40)
    planted = [(path_voxels(), [PLANTED["path"]]), (CORNER_PAIR, [PLANTED["corner"]]), (FACE_PAIR, list(PLANTED["face"]))]
    for voxels, _ in planted:                                           # a margin of one voxel that is outside in every mode
        for px, py, pz in voxels:
            lab[pz - 1:pz + 2, py - 1:py + 2, px - 1:px + 2] = 0
            d[pz - 1:pz + 2, py - 1:py + 2, px - 1:px + 2] = 0
    for voxels, ids in planted:
        for k, (px, py, pz) in enumerate(voxels):
            lab[pz, py, px] = ids[k % len(ids)]
            d[pz, py, px] = 255
    (cx, cy, cz), (sx, sy, sz) = CHECKER
    box = (slice(cz, cz + sz), slice(cy, cy + sy), slice(cx, cx + sx))
    even = (x[box] + y[box] + z[box]) % 2 == 0
    lab[box] = np.where(even, PLANTED["checker"], 0)
    d[box] = np.where(even, 255, 0)
    if kind == "u16":
        d = d.astype(np.uint16) * np.uint16(251)
    if kind == "f32":
        d = d.astype(f32) * f32(0.37) - f32(20.0)
        flat = d.reshape(-1)
        # inside the window of either LOD: even coordinates around the centre
        zz, yy, xx = (2 * rng.integers(c // 2 - 3, c // 2 + 3, 90) for c in (36, 30, 84))
        at = (zz * 64 + yy) * 128 + xx
        flat[at[:30]], flat[at[30:60]], flat[at[60:]] = np.nan, np.inf, -np.inf
    pairs = [(d, lab), (d[::2, ::2, ::2].copy(), lab[::2, ::2, ::2].copy())]
    if kind == "nolabels":
        pairs = [(p, None) for p, _ in pairs]
    return pairs


def spec_of(kind):
    spec = testing.synthetic_spec(64, 32, 32, pairs=volumes(kind),
                                  chunk_shapes=[(8, 8, 8), (4, 4, 4)], ring_shapes=[(5, 2, 9), (5, 3, 9)])
    spec.centers = [(CENTRE, None)]
    return spec


def checkerboard_spec():
    """A 128 x 64 x 64 checkerboard of label 1 (x, y, z extents), the whole of it resident: 2^18 components of one voxel
    under 6-connectivity."""
    z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(128), indexing="ij")
    lab = ((x + y + z) % 2 == 0).astype(np.uint32)
    d = (lab * 200).astype(np.uint8)
    spec = testing.synthetic_spec(64, 32, 32, pairs=[(d, lab)], chunk_shapes=[(8, 8, 8)], ring_shapes=[(8, 8, 16)])
    spec.centers = [((63.5, 31.5, 31.5), None)]
    return spec
