"""What the numpy float32 twins of the slice, slab, composite and iso kernels share, each piece stated once, as
csrc/ray_common.h does for the kernels: the frame's pixels, the LOD cascade with either sampling (``sample``), the
march's ray set-up (``setup_rays``), the plane chain of slices and slabs, the grey shading chain, the pick word, the
NDC depth, and the material and rings of a SceneSpec.  Everything is in the operation order include/svr.h states.
Ring contents come from the CPU ring restatement (``oracle.lmip.rings_of``): wrapped rings with their ROI offset, shape
and scale in shader order, textures [z][y][x], addressed like ``oracle/lmip_numpy.py``'s ``texel_index``."""
import numpy as np

from oracle import lmip

f32 = np.float32
DISCARD, MISS, HIT = 0, 1, 2


def material_of(spec_material, colors=None):
    """The uniforms the four kernels read, from a SceneSpec material dict (defaults of oracle.lmip)."""
    m = dict(lmip.DEFAULT_MATERIAL)
    m.update(spec_material)
    cols = colors if colors is not None else (m["colors"] if m["colors"] is not None else lmip.DEFAULT_COLORS)
    return dict(clim=m["clim"], gamma=m["gamma"], opacity=m["opacity"], colors=np.array([c[:2] for c in cols], f32),
                clipping_planes=m["clipping_planes"], clipping_mode=m["clipping_mode"])


def rings_of_spec(spec, vol=None, rings=None):
    """(volume, rings) of a SceneSpec after its ``center_on_position`` calls, unless the caller has them."""
    vol = vol or lmip.oracle_volume(spec)
    return vol, (lmip.rings_of(vol) if rings is None else rings)


def matrices_of(volume, camera):
    """The six row-major mat4 of svr_camera for a SubVolume (its current world transform) and a camera."""
    w = volume.world
    m = {"world": w.matrix, "world_inv": w.inverse_matrix, "cam": camera.view_matrix, "cam_inv": camera.camera_matrix,
         "proj": camera.projection_matrix, "proj_inv": camera.projection_matrix_inverse}
    return {k: np.asarray(v, np.float32) for k, v in m.items()}


def frame_pixels(width, height, region=None):
    """Frame pixel (x, y) of every output pixel, through svr_frame (padding rows fall outside the frame)."""
    if region is None:
        x0, y0, ow, oh, bh, bp = 0, 0, width, height, height, height
    else:
        x0, y0, ow, oh = region.x0, region.y0, region.out_w, region.out_h
        bh, bp = (region.band_h or oh), (region.band_pitch or oh)
    r, c = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    return x0 + c, y0 + (r // bh) * bp + (r % bh)


def flags_of(hit, frag):
    return np.where(hit, HIT, np.where(frag, MISS, DISCARD)).astype(np.uint8)


# ---- small vector algebra, in the contract's association
def _mv(m, x, y, z, w):
    """M * (x, y, z, w) as ((m0 x + m1 y) + m2 z) + m3 w; ``m`` row-major f32."""
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] * w for r in range(4)]


def _mm(a, b):
    out = np.zeros((4, 4), f32)
    for c in range(4):
        col = _mv(a, b[0, c], b[1, c], b[2, c], b[3, c])
        for r in range(4):
            out[r, c] = col[r]
    return out


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unit(v, fallback):
    """v / sqrtf(dot(v, v)) per component, ``fallback`` where the length is 0 or not finite."""
    ln = np.sqrt(_dot(v, v))
    ok = (ln > 0) & np.isfinite(ln)
    safe = np.where(ok, ln, f32(1.0))
    return [np.where(ok, v[k] / safe, fallback[k]) for k in range(3)]


# ---- the LOD cascade
def sample(rings, dd, allowed=None, linear=False):
    """The sample at arrays of data points ``dd`` = [dx, dy, dz] (f32), from the first LOD whose window holds the
    truncated coordinate: value, label, and that LOD (int32; -1: none, value and label are 0 there).  The value is
    the wrapped texel, or with ``linear`` the linear sample of svr.h taken inside that LOD; the label is the texel's
    either way.  ``allowed``: the points to look at (default all)."""
    shape = dd[0].shape
    value = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, -1, np.int32)
    with np.errstate(all="ignore"):
        for n, r in enumerate(rings):
            s = [dd[k] * f32(r["scale"][k]) for k in range(3)]
            ic = s if allowed is None else [np.where(allowed, s[k], f32(0)) for k in range(3)]
            ic = [c.astype(np.int32) for c in ic]                                         # trunc, like (int) in the kernels
            sel = lod < 0
            if allowed is not None:
                sel &= allowed
            for k in range(3):
                sel &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
            if not sel.any():
                continue
            rz, ry, rx = r["density"].shape
            ext = (rx, ry, rz)
            density = np.asarray(r["density"])
            texel = (ic[2][sel] % rz, ic[1][sel] % ry, ic[0][sel] % rx)
            label[sel] = np.asarray(r["labels"])[texel].astype(np.uint32)
            lod[sel] = n
            if not linear:
                value[sel] = density[texel].astype(f32)
                continue
            i0, i1, fr = [], [], []
            for k in range(3):
                p = s[k][sel] - f32(0.5)
                b = np.floor(p)
                fr.append(p - b)
                lo, hi = r["offset"][k], r["offset"][k] + r["shape"][k] - 1
                j = b.astype(np.int64)
                i0.append(np.clip(j, lo, hi) % ext[k])
                i1.append(np.clip(j + 1, lo, hi) % ext[k])

            def v(zi, yi, xi):
                return density[zi, yi, xi].astype(f32)

            fx, fy, fz = fr
            c = {}
            for zk, zi in ((0, i0[2]), (1, i1[2])):
                for yk, yi in ((0, i0[1]), (1, i1[1])):
                    a, b = v(zi, yi, i0[0]), v(zi, yi, i1[0])
                    c[(yk, zk)] = a + fx * (b - a)
            c0 = c[(0, 0)] + fy * (c[(1, 0)] - c[(0, 0)])
            c1 = c[(0, 1)] + fy * (c[(1, 1)] - c[(0, 1)])
            value[sel] = c0 + fz * (c1 - c0)
    return value, label, lod


# ---- rays: the march's set-up, and what the ray modes write for a point of a ray
def setup_rays(M, size, mat, W, H, region):
    """The march's ``setup_ray`` (march_kernel.hip) for every output pixel of ``region``: frag, nsteps, start, step,
    plus the matrices the outputs need."""
    world = np.asarray(M["world"], f32)
    ndc_to_data = _mm(_mm(np.asarray(M["world_inv"], f32), np.asarray(M["cam_inv"], f32)), np.asarray(M["proj_inv"], f32))
    pc = _mm(np.asarray(M["proj"], f32), np.asarray(M["cam"], f32))
    size = [f32(v) for v in size]
    rel = f32(min(max(np.sqrt(f32(max(size))) / f32(20.0), f32(0.1)), f32(0.8)))

    x, y = frame_pixels(W, H, region)
    frag = (x < W) & (y < H)
    px = (f32(2.0) * (x.astype(f32) + f32(0.5))) / f32(W) - f32(1.0)
    py = f32(1.0) - (f32(2.0) * (y.astype(f32) + f32(0.5))) / f32(H)
    one = np.ones_like(px)
    n4 = _mv(ndc_to_data, px, py, -one, one)
    f4 = _mv(ndc_to_data, px, py, one, one)
    far = [f4[k] / f4[3] for k in range(3)]
    near = [n4[k] / n4[3] for k in range(3)]
    d = [far[k] - near[k] for k in range(3)]
    ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ray = [d[k] / ln for k in range(3)]
    t1 = [(f32(-0.5) - near[k]) / ray[k] for k in range(3)]
    t2 = [((size[k] - f32(0.5)) - near[k]) / ray[k] for k in range(3)]
    tmax = [np.fmax(t1[k], t2[k]) for k in range(3)]
    tmin = [np.fmin(t1[k], t2[k]) for k in range(3)]
    t_exit = np.fmin(np.fmin(tmax[0], tmax[1]), tmax[2])
    t_enter = np.fmax(np.fmax(tmin[0], tmin[1]), tmin[2])
    frag &= t_enter <= t_exit
    back = [near[k] + ray[k] * t_exit for k in range(3)]
    bw = _mv(world, back[0], back[1], back[2], one)
    bc = _mv(pc, bw[0], bw[1], bw[2], bw[3])
    frag &= (bc[3] > 0) & (bc[2] >= 0) & (bc[2] <= bc[3])
    planes = np.array(mat.get("clipping_planes", ()), f32).reshape(-1, 4)
    if len(planes):
        behind = [((bw[0] * p[0] + bw[1] * p[1]) + bw[2] * p[2]) < p[3] for p in planes]
        if str(mat.get("clipping_mode", "ANY")).upper() == "ALL":
            frag &= ~np.logical_and.reduce(behind)
        else:
            frag &= ~np.logical_or.reduce(behind)
    nb = [near[k] - back[k] for k in range(3)]
    dist = (nb[0] * ray[0] + nb[1] * ray[1]) + nb[2] * ray[2]
    for k in range(3):
        dist = np.fmax(dist, np.fmin((f32(-0.5) - back[k]) / ray[k], (size[k] - f32(0.5) - back[k]) / ray[k]))
    front = [back[k] + ray[k] * dist for k in range(3)]
    nf = -dist / rel + f32(0.5)
    frag &= nf >= 1.0
    nf = np.where(frag, np.fmin(nf, f32(16777216.0)), f32(1.0))
    nsteps = nf.astype(np.int32)
    nstepsf = nsteps.astype(f32)
    start = [(front[k] + f32(0.5)) / size[k] for k in range(3)]
    step = [((back[k] - front[k]) / size[k]) / nstepsf for k in range(3)]
    return dict(frag=frag, nsteps=nsteps, start=start, step=step, world=world, pc=pc, size=size, shape=x.shape)


def ndc_depth(world, pc, c):
    """The depth plane's value for normalised points ``c`` of rays."""
    wp = _mv(world, c[0] - f32(0.5), c[1] - f32(0.5), c[2] - f32(0.5), np.ones_like(c[0]))
    ndc = _mv(pc, wp[0], wp[1], wp[2], wp[3])
    return ndc[2] / np.fmax(ndc[3], f32(0.001))


def pick_word(c, pick_id):
    """The pick word for normalised points ``c``: the id in bits 0-19, three 14-bit coordinates above it."""
    word = np.full(len(c[0]), min(int(pick_id), 0xFFFFF), np.uint64)
    for k, shift in enumerate((20, 34, 48)):
        fk = (c[k] * f32(16383.0)).astype(np.float64)
        u = np.where(fk > 0, np.minimum(np.floor(np.nan_to_num(fk, nan=0.0)), 16383.0), 0.0).astype(np.uint64)
        word |= u << np.uint64(shift)
    return word


def label_rgb(mat, label, v):
    """hsv_to_rgb of the material's (hue, saturation) of each label with the value ``v``."""
    colors = np.asarray(mat["colors"], f32)
    hs = colors[label % np.uint32(len(colors))]
    return hsv_to_rgb(hs[:, 0], hs[:, 1], v)


def hsv_to_rgb(h, s, v):
    """hsv_selection.wgsl:7-41, arrays of f32."""
    h6 = h * f32(6.0)
    fl = np.floor(h6)
    sector = fl.astype(np.int32)
    fr = h6 - fl
    p = v * (f32(1.0) - s)
    q = v * (f32(1.0) - s * fr)
    t = v * (f32(1.0) - s * (f32(1.0) - fr))
    conds = [sector == k for k in range(5)]
    r = np.select(conds, [v, q, p, p, t], v)
    g = np.select(conds, [t, v, v, q, p], p)
    b = np.select(conds, [p, p, t, v, v], q)
    grey = s == 0
    return np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)


# ---- planes: what slices and slabs share
def plane_points(world_inv, size, origin, u, v, W, H, region):
    """pixel -> p -> q of svr_slice for every output pixel of ``region``: (world_inv and size in f32, q, in_frame)."""
    m = np.asarray(world_inv, f32).reshape(4, 4)
    size = [f32(s) for s in size]
    o, u, v = [f32(c) for c in origin], [f32(c) for c in u], [f32(c) for c in v]
    x, y = frame_pixels(W, H, region)
    in_frame = (x < W) & (y < H)
    fx = (x.astype(f32) + f32(0.5)) - f32(0.5) * f32(W)
    fy = (y.astype(f32) + f32(0.5)) - f32(0.5) * f32(H)
    p = [(o[k] + fx * u[k]) + fy * v[k] for k in range(3)]
    q = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] * f32(1.0) for k in range(3)]
    return m, size, q, in_frame


def data_points(q, size, in_frame):
    """q -> dx, and which pixels of the frame have theirs inside the volume."""
    dx = [((q[k] + f32(0.5)) / size[k]) * size[k] for k in range(3)]
    inside = in_frame.copy()
    for k in range(3):
        inside &= (dx[k] >= 0) & (dx[k] < size[k])
    return dx, inside


def shade_grey(value, label, hit, inside, mat, srgb):
    """The rgba plane of slices and slabs: clim, gamma, sRGB decode, then the label's hue and saturation; opaque black
    inside the volume where no LOD holds the point, zero outside."""
    rgba = np.zeros(hit.shape + (4,), f32)
    rgba[inside & ~hit] = (0, 0, 0, 1)
    if hit.any():
        s = (value[hit] - f32(mat["clim"][0])) / (f32(mat["clim"][1]) - f32(mat["clim"][0]))
        if f32(mat["gamma"]) != f32(1.0):
            s = np.power(s, f32(mat["gamma"]), dtype=f32)
        if srgb:
            s = np.where(s <= f32(0.04045), s / f32(12.92), np.power((s + f32(0.055)) / f32(1.055), f32(2.4), dtype=f32))
        rgb = label_rgb(mat, label[hit], s.astype(f32))
        rgba[hit] = np.stack([*rgb, np.full_like(rgb[0], f32(mat["opacity"]))], axis=-1)
    return rgba
