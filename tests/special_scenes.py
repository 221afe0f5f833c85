"""Inputs shared by the CPU and GPU tiers of the special-value tests (tests/test_special_values.py,
tests/test_gpu_special_values.py): one float32 volume at three LODs whose voxels hold what a float ring may hold and
no other scene of the suite does — a smooth SIGNED field (about 45 % negative, |min| > max) with NaN, +-inf, -0.0, a
subnormal and +-3e38 planted in it — and the views, materials and mode settings that take those values through the
march, the slice, slab, composite and iso kernels.

Geometry.  64^3 / 32^3 / 16^3 voxels in 8^3 chunks.  The windows are nested shells, 32^3 of LOD 0, 24^3 of LOD 1 (48^3
fine voxels) and the whole of LOD 2, centred off the chunk grid so that LOD 0 and LOD 1 wrap around their rings on
every axis; every ring is whole macro cells of 8^3 slots.

Planting (array order [z, y, x]; the boxes are the constants below).  Per LOD and at that LOD's own positions: single voxels
of each special value; an 8^3 block of NaN on the macro-cell grid (its cell maximum is 0), one that straddles eight
cells, and an aligned 8^3 block of -inf (in LOD 0 with a plate of +inf on one face); in LOD 0 also a two-voxel NaN box
at the inside camera's eye with a +inf and a -inf box behind it.  At the same place in every LOD, because rays must meet them whichever LOD
serves a voxel: a NaN patch over the quarter of the x = 0 face through which the outside camera's rays enter (rays
whose first sample is NaN), a slab of zeros behind another quarter of that face whose z layers alternate between -0.0
and +0.0 (runs that start and stay at zero; columns along z in which -0.0 ties +0.0), and an
8 x 8 bundle of voxel columns that is NaN from face to face along each axis (orthographic axis views with rays that
have no non-NaN sample)."""
import numpy as np

import ortho_scenes as ortho
from oracle import lmip
from twin_common import data_points, plane_points, sample
from sub_volume_renderer_amd import SubVolume, TransferFunction, testing

f32 = np.float32
N = 64
CHUNKS = [(8, 8, 8), (8, 8, 8), (8, 8, 8)]
RINGS = [(4, 4, 4), (3, 3, 3), (2, 2, 2)]
CENTRE = (37.0, 39.0, 35.0)
SUBNORMAL = np.float32(1e-41)
BIG = np.float32(3e38)
SINGLES = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), SUBNORMAL, BIG, -BIG)
N_SINGLES = 40                       # voxels of each special value per LOD

# boxes in FINE voxels, (z0, z1, y0, y1, x0, x1); a LOD holds them shifted right by its level
FACE_NAN = (32, 64, 32, 64, 0, 4)
FACE_NEG_ZERO = (32, 64, 0, 32, 0, 8)
COLUMNS = {"x": (16, 24, 24, 32, 0, 64), "y": (40, 48, 0, 64, 40, 48), "z": (0, 64, 40, 48, 16, 24)}
POS_INF_PLATE = (32, 34, 24, 32, 48, 56)   # LOD 0: two layers of +inf on the -inf block, so that columns along z hold both
# LOD 0, ahead of the inside camera's eye (37.9, 34.7, 18.7), which looks along (0.6, 0.3, 0.74): the middle of its frame
# passes a NaN box
# one voxel on and meets a +inf and a -inf box behind it, within the eleven samples of an LMIP run that starts at the eye
EYE_NAN = (19, 21, 34, 36, 38, 40)
EYE_POS_INF = (21, 23, 35, 37, 40, 42)
EYE_NEG_INF = (21, 23, 33, 35, 40, 42)
# boxes in the LOD's OWN voxels
BLOCKS = {
    0: dict(nan_aligned=(32, 40, 32, 40, 24, 32), nan_straddle=(20, 28, 44, 52, 36, 44), neg_inf=(24, 32, 24, 32, 48, 56)),
    1: dict(nan_aligned=(24, 32, 8, 16, 8, 16), nan_straddle=(20, 28, 12, 20, 20, 28), neg_inf=(24, 32, 24, 32, 24, 32)),
    2: dict(nan_aligned=(0, 8, 0, 8, 8, 16), nan_straddle=(4, 12, 4, 12, 4, 12), neg_inf=(8, 16, 0, 8, 8, 16)),
}


def _box(a, b, level=0):
    z0, z1, y0, y1, x0, x1 = [(v >> level) for v in b]
    return a[z0:max(z1, z0 + 1), y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)]


def smooth_field(n):
    """A smooth signed field sampled at voxel centres of an n^3 grid over the unit cube: 45 % negative by
    construction (the 45 % quantile is subtracted), negative values stretched by 1.5 so that |min| > max."""
    t = (np.arange(n, dtype=np.float64) + 0.5) / n
    z, y, x = np.meshgrid(t, t, t, indexing="ij")
    g = 40.0 * np.sin(2 * np.pi * (1.3 * x + 0.4)) * np.cos(2 * np.pi * 0.9 * y) + 25.0 * np.sin(2 * np.pi * (1.1 * z + 0.2 * x))
    g = g - np.quantile(g, 0.45)
    return np.where(g < 0, 1.5 * g, g).astype(np.float32)


_pairs = None


def pairs():
    """[(density f32, labels u32)] per LOD; built once, shared, never written to."""
    global _pairs
    if _pairs is not None:
        return _pairs
    out = []
    for l in range(3):
        n = N >> l
        rng = np.random.default_rng(9100 + l)
        d = smooth_field(n)
        for value in SINGLES:
            idx = rng.integers(0, n, (N_SINGLES, 3))
            d[idx[:, 0], idx[:, 1], idx[:, 2]] = value
        _box(d, BLOCKS[l]["neg_inf"])[...] = -np.inf
        if l == 0:
            _box(d, POS_INF_PLATE)[...] = np.inf
            _box(d, EYE_POS_INF)[...] = np.inf
            _box(d, EYE_NEG_INF)[...] = -np.inf
            _box(d, EYE_NAN)[...] = np.nan
        _box(d, BLOCKS[l]["nan_aligned"])[...] = np.nan             # (the 16^3 of LOD 2 has no room to keep the blocks apart:
        _box(d, BLOCKS[l]["nan_straddle"])[...] = np.nan            # there the straddling block takes a corner of the other two)
        _box(d, FACE_NEG_ZERO, l)[0::2] = -0.0                  # z layers alternate: -0.0 ties +0.0 along z
        _box(d, FACE_NEG_ZERO, l)[1::2] = 0.0
        _box(d, FACE_NAN, l)[...] = np.nan
        for b in COLUMNS.values():
            _box(d, b, l)[...] = np.nan
        lab = rng.integers(0, 2**32, (n, n, n), dtype=np.uint64).astype(np.uint32)
        lab[rng.random((n, n, n)) < 0.1] = 0
        d.setflags(write=False)
        lab.setflags(write=False)
        out.append((d, lab))
    _pairs = out
    return out


COLORS = [(0.0, 1.0, 1.0), (0.3, 0.8, 1.0), (0.6, 1.0, 1.0), (0.9, 0.0, 1.0)]          # the last one is grey (s == 0)
CLIMS = {"wide": (-60.0, 60.0), "above": (10.0, 60.0)}                                 # "above": clim[0] over part of the data


def material(clim="wide", gamma=1.0, **kw):
    m = dict(lmip_threshold=20.0, lmip_fall_off=0.5, lmip_max_samples=10, fog_density=0.01, fog_color=(0.5, 0.5, 0.5),
             colors=COLORS, clim=CLIMS[clim], gamma=gamma)
    m.update(kw)
    return m


def spec_of(view, width=None, height=None, **mat):
    """view: "outside" / "inside" (the perspective cameras of testing.synthetic_spec) or an orthographic axis view
    "+x" .. "-z" at one pixel per voxel."""
    if view in ortho.AXES:
        spec = ortho.base_spec(pairs(), CHUNKS, RINGS, width or 64, height or 64, centre=CENTRE)
        spec.material = material(**mat)
        return ortho.axis_view(spec, view)
    spec = testing.synthetic_spec(N, width or 96, height or 80, inside=(view == "inside"), pairs=pairs(),
                                  chunk_shapes=CHUNKS, ring_shapes=RINGS)
    spec.material = material(**mat)
    spec.centers = [(CENTRE, None)]
    spec.ring_storage = "float32"
    return spec


VIEWS = ("outside", "inside", "+x", "+y", "+z")
ORTHO_VIEWS = ("+x", "+y", "+z")

# march modes: name -> material settings
MARCH = {
    "lmip+20": dict(lmip_threshold=20.0),
    "lmip-30": dict(lmip_threshold=-30.0),
    "lmip0": dict(lmip_threshold=0.0, lmip_max_samples=3),
    "lmip+inf": dict(lmip_threshold=float("inf")),
    "mip": dict(render_mode="mip"),
    "wavg": dict(render_mode="weighted_average", weight_falloff=0.02),
}
# shading: name -> (clim, gamma, colorspace)
SHADING = {"wide-g1-srgb": ("wide", 1.0, "srgb"), "above-g1.6-linear": ("above", 1.6, "linear"),
           "wide-g1.6-srgb": ("wide", 1.6, "srgb")}


def march_spec(view, mode, shading="wide-g1-srgb", **kw):
    clim, gamma, colorspace = SHADING[shading]
    spec = spec_of(view, clim=clim, gamma=gamma, **MARCH[mode], **kw)
    spec.colorspace = colorspace
    return spec


# ---- planes, slabs, transfer functions, iso settings ------------------------------------------------------------------
def planes(p=1.0):
    """(name, origin, u, v): the three axis planes through the window's centre and one oblique plane."""
    out = []
    o = tuple(np.array(CENTRE) + np.array([0.13, -0.21, 0.07]))
    for axis in ("z", "y", "x"):
        _, u, v = SubVolume.axis_slice_plane(axis, (0, 0, 0), p)
        out.append((axis, o, u, v))
    out.append(("oblique", o, tuple(p * np.array([0.8, 0.6, 0.0])), tuple(p * np.array([-0.36, 0.48, 0.8]))))
    return out


def centre_planes():
    """(name, origin, u, v, w): axis planes at pixel size 1 whose pixel centres are voxel centres (in-plane origin on
    half-integers for the even frame, the normal coordinate an integer) and whose unit step w keeps slab samples on
    them: inside LOD 0's window every fraction of the linear cell is exactly 0, so each of the seven other corners has
    weight 0.  The planes cut the NaN block, the +inf plate and the -inf block of LOD 0."""
    out = []
    for axis, o in (("z", (36.5, 39.5, 33.0)), ("y", (36.5, 33.0, 35.5)), ("x", (49.0, 39.5, 35.5))):
        _, u, v = SubVolume.axis_slice_plane(axis, (0, 0, 0), 1.0)
        out.append((axis, o, u, v, SLAB_W[axis]))
    return out


SLAB_W = {"z": (0.0, 0.0, 1.0), "y": (0.0, 1.0, 0.0), "x": (1.0, 0.0, 0.0), "oblique": (0.35, -0.5, 0.6)}
SLAB_SAMPLES = (1, 7, 16)
SLAB_MODES = ("max", "min", "mean")

TF_TINT = TransferFunction.from_points([(0.0, (0.1, 0.2, 0.9, 0.02)), (0.3, (0.2, 0.9, 0.3, 0.08)), (0.6, (1.0, 0.6, 0.1, 0.3)),
                                        (1.0, (1.0, 1.0, 1.0, 0.6))], size=64)
TF_PLAIN = TransferFunction.from_points([(0.0, (0.3, 0.1, 0.1, 0.05)), (0.5, (0.3, 0.3, 0.3, 0.0)), (1.0, (1.0, 0.5, 0.2, 0.9))],
                                        size=256)
COMPOSITES = [(TF_TINT, 0.99, True), (TF_PLAIN, 1.0, False)]               # (table, alpha cutoff, tint by label)

ISO_RUNS = [dict(level=25.0, iso_refine=4), dict(level=0.0, iso_refine=0), dict(level=-40.0, iso_refine=4, color_by_label=True),
            dict(level=float("-inf"), iso_refine=0)]
CUT = ([(0.8, -0.36, -0.48, float(0.8 * CENTRE[0] - 0.36 * CENTRE[1] - 0.48 * CENTRE[2]))], "ANY")   # opens the side towards "outside"


# ---- what the march samples, from the arrays alone --------------------------------------------------------------------
def rois(orac):
    out = []
    for b in orac.wrapping_buffers:
        u = b.uniform()
        out.append((tuple(int(v) for v in u["offset"]), tuple(int(v) for v in u["shape"])) if all(u["shape"]) else None)
    return out


def composite_f32(orac):
    """The finest-resolution volume the march samples (ortho_scenes.composite) with its float32 bits kept: value and
    label arrays indexed [z, y, x]."""
    val, lab = ortho.composite(pairs(), rois(orac))
    return val.astype(np.float32), lab


# ---- the samples of a slab's columns, as the slab twin takes them ------------------------------------------------------
def slab_columns(spec, orac, o, u, v, w, n, linear=False):
    """The N samples of every pixel's slab column, as the slab twin takes them: values [N, H, W] and which are held."""
    rings = lmip.rings_of(orac)
    m, size, q, in_frame = plane_points(spec.world().inverse_matrix, orac.volume_dimensions_shader, o, u, v, spec.width, spec.height, None)
    w = [f32(c) for c in w]
    dw = [(m[k, 0] * w[0] + m[k, 1] * w[1]) + m[k, 2] * w[2] for k in range(3)]
    half = f32(0.5) * f32(n - 1)
    vals, held = [], []
    for k in range(n):
        dx, inside = data_points([q[i] + (f32(k) - half) * dw[i] for i in range(3)], size, in_frame)
        val, _, lod = sample(rings, dx, inside, linear)
        vals.append(val)
        held.append(lod >= 0)
    return np.stack(vals), np.stack(held)


# ---- known answers of the orthographic axis views, from the voxel columns alone ---------------------------------------
def column_answers(spec, orac, mode, thr=None):
    """Per pixel of an axis view at one pixel per voxel: flags, winning voxel's value and label and its index along the
    ray's axis (-1 without a hit), and the pixels judged (in the volume, centre off every voxel face).  MIP: the first
    argmax of |v| over the column's non-NaN voxels; "first": the first voxel with |v| >= thr (what an LMIP run starts
    from; a NaN fails the comparison).  A column without such a voxel is a MISS.  Views down +x / +y / +z only: their
    rays take every sample inside the volume (a ray down a negative axis takes its first one on the far face, where no
    LOD holds it and the sample is 0)."""
    a, sign, (iu, iv), inside, edge = ortho.columns(spec)
    assert sign > 0
    val, lab = composite_f32(orac)
    val_xyz, lab_xyz = val.transpose(2, 1, 0), lab.transpose(2, 1, 0)
    H, W = inside.shape
    flags = np.zeros((H, W), np.uint8)
    value = np.zeros((H, W), np.float32)
    label = np.zeros((H, W), np.uint32)
    index = np.full((H, W), -1)
    judged = inside & ~edge
    for j, i in zip(*np.nonzero(judged)):
        col = ortho.column_of(val_xyz, a, sign, iu[j, i], iv[j, i])
        mag = np.abs(col)
        ok = ~np.isnan(col) if mode == "mip" else mag >= np.float32(thr)      # NaN >= thr is False
        if not ok.any():
            flags[j, i] = 1
            continue
        k = int(np.argmax(np.where(ok, mag, -1.0))) if mode == "mip" else int(np.argmax(ok))
        flags[j, i], value[j, i], index[j, i] = 2, col[k], k
        label[j, i] = ortho.column_of(lab_xyz, a, sign, iu[j, i], iv[j, i])[k]
    return dict(flags=flags, value=value, label=label, index=index, judged=judged, axis=a, columns=(iu, iv),
                val_xyz=val_xyz, lab_xyz=lab_xyz)


def lmip_walk(col, thr, fall, maxs):
    """raycast.wgsl's run over one voxel column of an axis view down a positive axis, in scalar float32: sample i of
    nsteps = int(n / rel + 0.5) lies in voxel int((i * (1 / nsteps)) * n), rel = clamp(sqrt(n) / 20, 0.1, 0.8).  Returns
    (winning voxel or -1, samples executed)."""
    f = np.float32
    n = len(col)
    rel = f(min(max(np.sqrt(f(n)) / f(20.0), f(0.1)), f(0.8)))
    nsteps = int(f(n) / rel + f(0.5))
    step = (f(n) / f(n)) / f(nsteps)
    found, lmax, since, win = False, f(0.0), 0, -1
    for i in range(nsteps):
        k = int((f(i) * step) * f(n))
        mag = abs(f(col[k]))
        if not found:
            if mag >= f(thr):
                found, lmax, win = True, mag, k
            continue
        since += 1
        if mag > lmax:
            lmax, win = mag, k
        if since >= maxs or mag < lmax * f(fall):
            return win, i + 1
    return win, nsteps


def depth_bounds(spec, index, a):
    """The orthographic NDC depth interval of a hit in voxel `index` along axis `a` (test_gpu_ortho._depth_bounds)."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    pc = M["proj"] @ M["cam"] @ M["world"]
    size = ortho.size_xyz(spec)[a]

    def depth(t):
        p = np.zeros((4,) + t.shape)
        p[a], p[3] = t - 0.5, 1.0
        c = np.einsum("rc,c...->r...", pc, p)
        return c[2] / c[3]

    d0, d1 = depth(index / size), depth((index + 1) / size)
    return np.minimum(d0, d1), np.maximum(d0, d1)
