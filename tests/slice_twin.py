"""numpy float32 restatement of svr_slice (include/svr.h, "cross-section views"), in the operation order stated
there.  Ring contents come from the CPU ring restatement (``oracle.lmip.rings_of``): wrapped rings with their ROI
offset, shape and scale, addressed like ``oracle/lmip_numpy.py``'s ``texel_index``."""
import numpy as np

from oracle import lmip

f32 = np.float32
DISCARD, MISS, HIT = 0, 1, 2


def material_of(spec_material):
    """The colour uniforms of a SceneSpec material dict (defaults of oracle.lmip)."""
    m = dict(lmip.DEFAULT_MATERIAL)
    m.update(spec_material)
    colors = m["colors"] if m["colors"] is not None else lmip.DEFAULT_COLORS
    return dict(clim=m["clim"], gamma=m["gamma"], opacity=m["opacity"], colors=np.array([c[:2] for c in colors], f32))


def frame_pixels(width, height, region=None):
    """Frame pixel (x, y) of every output pixel, through svr_frame (padding rows fall outside the frame)."""
    if region is None:
        x0, y0, ow, oh, bh, bp = 0, 0, width, height, height, height
    else:
        x0, y0, ow, oh = region.x0, region.y0, region.out_w, region.out_h
        bh, bp = (region.band_h or oh), (region.band_pitch or oh)
    r, c = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    return x0 + c, y0 + (r // bh) * bp + (r % bh)


def slice_twin(rings, world_inv, size, origin, u, v, width, height, material, colorspace_srgb=True, region=None):
    """``rings``: oracle.lmip.rings_of(...) (shader-order offset / shape / scale, textures [z][y][x]);
    ``world_inv``: row-major 4x4 (cast to f32 here); ``size``: volume_dimensions in shader order.
    Returns dict(rgba, depth, label, flags, value, lod) for the output pixels of ``region`` (default: the frame)."""
    with np.errstate(all="ignore"):
        return _slice(rings, world_inv, size, origin, u, v, width, height, material, colorspace_srgb, region)


def _slice(rings, world_inv, size, origin, u, v, W, H, mat, srgb, region):
    m = np.asarray(world_inv, f32).reshape(4, 4)
    size = [f32(s) for s in size]
    o, u, v = [f32(c) for c in origin], [f32(c) for c in u], [f32(c) for c in v]
    x, y = frame_pixels(W, H, region)
    in_frame = (x < W) & (y < H)
    fx = (x.astype(f32) + f32(0.5)) - f32(0.5) * f32(W)
    fy = (y.astype(f32) + f32(0.5)) - f32(0.5) * f32(H)
    p = [(o[k] + fx * u[k]) + fy * v[k] for k in range(3)]
    q = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] * f32(1.0) for k in range(3)]
    dx = [((q[k] + f32(0.5)) / size[k]) * size[k] for k in range(3)]
    inside = in_frame.copy()
    for k in range(3):
        inside &= (dx[k] >= 0) & (dx[k] < size[k])

    shape = x.shape
    value = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, 255, np.uint8)
    done = ~inside
    for l, r in enumerate(rings):
        ic = [np.where(inside, dx[k] * f32(r["scale"][k]), 0).astype(np.int64) for k in range(3)]   # trunc (dx >= 0)
        inb = ~done
        for k in range(3):
            inb &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
        if inb.any():
            rz, ry, rx = r["density"].shape
            zi, yi, xi = ic[2][inb] % rz, ic[1][inb] % ry, ic[0][inb] % rx
            value[inb] = np.asarray(r["density"], f32)[zi, yi, xi]
            label[inb] = np.asarray(r["labels"]).astype(np.uint32)[zi, yi, xi]
            lod[inb] = l
        done |= inb
    hit = lod != 255
    flags = np.where(hit, HIT, np.where(inside, MISS, DISCARD)).astype(np.uint8)
    rgba = np.zeros(shape + (4,), f32)
    rgba[inside & ~hit] = (0, 0, 0, 1)
    if hit.any():
        s = (value[hit] - f32(mat["clim"][0])) / (f32(mat["clim"][1]) - f32(mat["clim"][0]))
        if f32(mat["gamma"]) != f32(1.0):
            s = np.power(s, f32(mat["gamma"]), dtype=f32)
        if srgb:
            s = np.where(s <= f32(0.04045), s / f32(12.92), np.power((s + f32(0.055)) / f32(1.055), f32(2.4), dtype=f32))
        colors = np.asarray(mat["colors"], f32)
        hs = colors[label[hit] % np.uint32(len(colors))]
        rgb = hsv_to_rgb(hs[:, 0], hs[:, 1], s.astype(f32))
        rgba[hit] = np.stack([*rgb, np.full_like(rgb[0], f32(mat["opacity"]))], axis=-1)
    return dict(rgba=rgba, depth=np.zeros(shape, f32), label=label, flags=flags, value=value, lod=lod)


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


def twin_of_spec(spec, origin, u, v, width, height, *, world_inv=None, region=None, vol=None, rings=None):
    """The restatement for a SceneSpec's volume after its ``center_on_position`` calls."""
    vol = vol or lmip.oracle_volume(spec)
    if rings is None:
        rings = lmip.rings_of(vol)
    if world_inv is None:
        world_inv = spec.world().inverse_matrix
    return slice_twin(rings, world_inv, vol.volume_dimensions_shader, origin, u, v, width, height,
                      material_of(spec.material), colorspace_srgb=(spec.colorspace == "srgb"), region=region)
