"""numpy float32 restatement of svr_slab (include/svr.h, "thick-slab projections"), in the operation order stated
there.  The per-pixel chain up to q and the shading are svr_slice's (tests/slice_twin.py); ring contents come from
the CPU ring restatement (``oracle.lmip.rings_of``), addressed like ``slice_twin``."""
import numpy as np

from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, frame_pixels, hsv_to_rgb, material_of

f32 = np.float32
MODES = ("max", "min", "mean")


def slab_twin(rings, world_inv, size, origin, u, v, w, samples, mode, width, height, material, colorspace_srgb=True,
              region=None):
    """``rings``: oracle.lmip.rings_of(...) (or dicts of the same keys); ``world_inv``: row-major 4x4 (cast to f32
    here); ``size``: volume_dimensions in shader order.  Returns dict(rgba, depth, label, flags, value, lod)."""
    assert mode in MODES and 1 <= samples <= 4096
    with np.errstate(all="ignore"):
        return _slab(rings, world_inv, size, origin, u, v, w, samples, mode, width, height, material, colorspace_srgb,
                     region)


def w_len_of(w):
    """|w| as the caller passes it: the float32 of the float64 norm of the float32 vector."""
    return f32(np.linalg.norm(np.array([f32(c) for c in w], np.float64)))


def lookup(rings, dx, inside):
    """value / label / lod of the first LOD whose ROI holds dx (slice_twin's rule); lod 255 where none does."""
    shape = dx[0].shape
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
    return value, label, lod


def _slab(rings, world_inv, size, origin, u, v, w, N, mode, W, H, mat, srgb, region):
    m = np.asarray(world_inv, f32).reshape(4, 4)
    size = [f32(s) for s in size]
    o, u, v, w = [f32(c) for c in origin], [f32(c) for c in u], [f32(c) for c in v], [f32(c) for c in w]
    x, y = frame_pixels(W, H, region)
    in_frame = (x < W) & (y < H)
    fx = (x.astype(f32) + f32(0.5)) - f32(0.5) * f32(W)
    fy = (y.astype(f32) + f32(0.5)) - f32(0.5) * f32(H)
    p = [(o[k] + fx * u[k]) + fy * v[k] for k in range(3)]
    q = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] * f32(1.0) for k in range(3)]
    dw = [(m[k, 0] * w[0] + m[k, 1] * w[1]) + m[k, 2] * w[2] for k in range(3)]
    half = f32(0.5) * f32(N - 1)

    shape = x.shape
    hits = np.zeros(shape, np.int64)
    total = np.zeros(shape, f32)
    best = np.zeros(shape, f32)
    best_k = np.zeros(shape, np.int64)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, 255, np.uint8)
    inside_any = np.zeros(shape, bool)
    for k in range(N):
        t = f32(k) - half
        qk = [q[i] + t * dw[i] for i in range(3)]
        dx = [((qk[i] + f32(0.5)) / size[i]) * size[i] for i in range(3)]
        inside = in_frame.copy()
        for i in range(3):
            inside &= (dx[i] >= 0) & (dx[i] < size[i])
        val, lab, lo = lookup(rings, dx, inside)
        hit = lo != 255
        wins = (val < best) if mode == "min" else (val > best)
        take = hit & ((hits == 0) | wins)
        best[take], best_k[take], label[take], lod[take] = val[take], k, lab[take], lo[take]
        total[hit] = total[hit] + val[hit]
        hits += hit
        inside_any |= inside
    hit = hits > 0
    value = np.zeros(shape, f32)
    if mode == "mean":
        value[hit] = total[hit] / hits[hit].astype(f32)
    else:
        value[hit] = best[hit]
    depth = np.zeros(shape, f32)
    depth[hit] = (best_k[hit].astype(f32) - half) * w_len_of(w)
    flags = np.where(hit, HIT, np.where(inside_any, MISS, DISCARD)).astype(np.uint8)
    rgba = np.zeros(shape + (4,), f32)
    rgba[inside_any & ~hit] = (0, 0, 0, 1)
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
    return dict(rgba=rgba, depth=depth, label=np.where(hit, label, 0).astype(np.uint32), flags=flags, value=value,
                lod=np.where(hit, lod, 255).astype(np.uint8))


def twin_of_spec(spec, origin, u, v, w, samples, mode, width, height, *, world_inv=None, region=None, vol=None,
                 rings=None):
    """The restatement for a SceneSpec's volume after its ``center_on_position`` calls."""
    vol = vol or lmip.oracle_volume(spec)
    if rings is None:
        rings = lmip.rings_of(vol)
    if world_inv is None:
        world_inv = spec.world().inverse_matrix
    return slab_twin(rings, world_inv, vol.volume_dimensions_shader, origin, u, v, w, samples, mode, width, height,
                     material_of(spec.material), colorspace_srgb=(spec.colorspace == "srgb"), region=region)
