"""Orthographic (parallel-ray) scenes shared by tests/test_oracle_lmip.py and tests/test_gpu_ortho.py, and the float64
geometry that shows which case a scene reaches: ray components that are exactly zero, pixel centres that lie exactly on
voxel faces or on the proxy box's faces (-0.5 and size - 0.5), and the voxel column behind each pixel.

The geometry is derived from the float32 matrices the kernel and the oracle receive (``SceneSpec.matrices()``), but in
float64 and with none of their code: for the scenes here every product is exact, so "exactly on a face" in float64 is
exactly on it in float32 too."""
import numpy as np

from sub_volume_renderer_amd import testing

AXES = {"+x": (0, 1.0), "-x": (0, -1.0), "+y": (1, 1.0), "-y": (1, -1.0), "+z": (2, 1.0), "-z": (2, -1.0)}


def size_xyz(spec):
    return np.array(spec.pairs[0][0].shape[::-1], np.float64)


def axis_view(spec, view, *, ppv=1, face=False, distance=None, screen_offset=(0.0, 0.0)):
    """Point `spec`'s orthographic camera along `view` ("+x", "-z", ...: the direction the rays travel) at
    ``ppv`` pixels per voxel.  The frame's extent is ``(width, height) / ppv`` world units.  The two screen-plane
    coordinates of the camera are chosen so that pixel centres fall in the middle of voxel columns (1 px per voxel)
    or a quarter voxel from their faces (2 px per voxel); ``face=True`` moves them by half a pixel, onto the
    voxel faces (and, where the frame is wider than the volume, onto the box faces).  ``screen_offset`` adds whole
    voxels.  Frame sizes must be powers of two so that NDC pixel centres are exact."""
    a, s = AXES[view]
    size = size_xyz(spec)
    for n in (spec.width, spec.height):
        assert n & (n - 1) == 0, "power-of-two frames keep every pixel centre exact"
    spec.projection = "orthographic"
    spec.ortho_size = (spec.width / ppv, spec.height / ppv)
    d = float(distance if distance is not None else 2.0 * size.max())
    pos = np.floor((size - 1.0) / 2.0)                      # an integer (voxel centre) on every axis
    others = [k for k in range(3) if k != a]
    # pixel centres sit at pos + (i + 1/2 - n/2) / ppv: for even n and an integer pos that is pos + k + 1/2 at
    # 1 px per voxel (every centre on a face) and pos + k +- 1/4 at 2 px per voxel (a quarter voxel inside)
    shift = {(1, False): 0.5, (1, True): 0.0, (2, False): 0.0, (2, True): 0.25}[(ppv, bool(face))]
    for k, o in zip(others, screen_offset):
        pos[k] += o + shift
    pos[a] = (size[a] - 1.0) / 2.0 - s * d
    tgt = pos.copy()
    tgt[a] += s
    spec.cam_position, spec.cam_target = tuple(float(v) for v in pos), tuple(float(v) for v in tgt)
    spec.depth_range = (1.0, 2.0 * d + 2.0)
    return spec


def pixel_rays(spec):
    """float64 near-plane points and unit directions of every pixel's ray in data coordinates, [3, H, W] each."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    n2d = M["world_inv"] @ M["cam_inv"] @ M["proj_inv"]
    W, H = spec.width, spec.height
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = 2 * (ii + 0.5) / W - 1, 1 - 2 * (jj + 0.5) / H

    def unproject(z):
        v = np.einsum("rc,chw->rhw", n2d, np.stack([px, py, np.full_like(px, z), np.ones_like(px)]))
        return v[:3] / v[3]

    near, far = unproject(-1.0), unproject(1.0)
    return near, (far - near) / np.linalg.norm(far - near, axis=0)


def direction_column(spec):
    """Column 2 of ndc_to_data as the kernel receives it (float32 entries, exact products in float64): the NDC-z
    coefficient, i.e. (up to scale) the direction every ray takes in data coordinates."""
    M = {k: np.asarray(v, np.float64) for k, v in spec.matrices().items()}
    return (M["world_inv"] @ M["cam_inv"] @ M["proj_inv"])[:3, 2]


def face_distance(coord):
    """Distance of a data coordinate to the nearest voxel face (faces at k - 0.5)."""
    f = coord + 0.5
    return np.abs(f - np.round(f))


def columns(spec, margin=1e-3):
    """For an axis-aligned orthographic view: the ray axis, its sign, and per pixel the voxel column (u, v indices on
    the two other axes in increasing axis order), whether the column lies in the volume, and whether the pixel centre
    is within `margin` voxel of a column face (excluded from known answers)."""
    near, ray = pixel_rays(spec)
    a = int(np.argmax(np.abs(ray[:, 0, 0])))
    assert np.all(np.delete(ray, a, axis=0) == 0.0), "not an axis-aligned view"
    sign = float(np.sign(ray[a, 0, 0]))
    others = [k for k in range(3) if k != a]
    size = size_xyz(spec)
    idx, inside, edge = [], np.ones(near.shape[1:], bool), np.zeros(near.shape[1:], bool)
    for k in others:
        c = near[k]
        i = np.floor(c + 0.5).astype(np.int64)
        idx.append(i)
        inside &= (i >= 0) & (i < size[k])
        edge |= face_distance(c) < margin
    return a, sign, idx, inside, edge


def composite(pairs, rois):
    """The volume the march samples, at the finest resolution: for each finest voxel the first LOD whose ROI holds
    it, at index >> l (sample_vol.wgsl:51-63); 0 / label 0 where no ROI does.  ``rois``: per LOD ((x, y, z) offset,
    (x, y, z) shape) in that LOD's voxels, or None."""
    shp = pairs[0][0].shape
    val = np.zeros(shp, np.float64)
    lab = np.zeros(shp, np.uint32)
    done = np.zeros(shp, bool)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shp], indexing="ij")
    for l, ((d, s), roi) in enumerate(zip(pairs, rois)):
        if roi is None:
            continue
        (ox, oy, oz), (sx, sy, sz) = roi
        x, y, z = xx >> l, yy >> l, zz >> l
        hold = (ox <= x) & (x < ox + sx) & (oy <= y) & (y < oy + sy) & (oz <= z) & (z < oz + sz) & ~done
        val[hold] = np.asarray(d)[z[hold], y[hold], x[hold]]
        if s is not None:
            lab[hold] = np.asarray(s)[z[hold], y[hold], x[hold]]
        done |= hold
    return val, lab


def column_of(vol_xyz, a, sign, u, v):
    """The voxel column (in ray order) of an [x, y, z]-indexed array along axis `a` at the other two indices."""
    sl = [None, None, None]
    others = [k for k in range(3) if k != a]
    sl[others[0]], sl[others[1]] = u, v
    sl[a] = slice(None)
    col = vol_xyz[tuple(sl)]
    return col if sign > 0 else col[::-1]


def base_spec(pairs, chunk_shapes, ring_shapes, width=32, height=32, centre=None, sizes=None, **material):
    size = np.array(pairs[0][0].shape[::-1], np.float64)
    c = tuple(float(v) for v in ((size - 1) / 2 if centre is None else centre))
    m = dict(lmip_threshold=128.0, lmip_fall_off=0.5, lmip_max_samples=10, fog_density=0.02, fog_color=(0.5, 0.5, 0.5),
             colors=[(0.0, 1.0, 1.0), (0.3, 0.8, 1.0), (0.6, 1.0, 1.0), (0.9, 0.5, 1.0)], clim=(0.0, 255.0))
    m.update(material)
    return testing.SceneSpec(pairs=list(pairs), chunk_shapes=list(chunk_shapes), ring_shapes=list(ring_shapes),
                             material=m, width=width, height=height, centers=[(c, sizes)])
