"""numpy float32 restatement of the linear sample (include/svr.h, "interpolation"), in the operation order stated
there, and the slice / slab / composite / iso definitions run with it.

``linear_sample`` is the definition itself.  slab_twin, composite_twin and iso_twin reach the rings through one
module-level ``lookup`` each and nothing else in their definitions changes under linear sampling, so they are reused as
they are with that one function exchanged for the duration of a call (``_sampling``); slice_twin does its lookup
inline, so the slice is restated here on slab_twin's pieces.  Ring contents come from the CPU ring restatement
(``oracle.lmip.rings_of``): wrapped rings with their ROI offset, shape and scale in shader order."""
import contextlib

import numpy as np

import composite_twin
import iso_twin
import slab_twin
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, frame_pixels, hsv_to_rgb, material_of

f32 = np.float32


def linear_sample(rings, dd, allowed=None):
    """The linear sample of svr.h for arrays of data points ``dd`` = [dx, dy, dz] (f32): value, the nearest sample's
    label, and the LOD that holds the point (-1: none; value and label are 0 there).  ``allowed``: points to look at."""
    shape = dd[0].shape
    value = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, -1, np.int32)
    allowed = np.ones(shape, bool) if allowed is None else allowed
    with np.errstate(all="ignore"):
        for n, r in enumerate(rings):
            s = [dd[k] * f32(r["scale"][k]) for k in range(3)]
            ic = [np.where(allowed, s[k], f32(0)).astype(np.int32) for k in range(3)]     # trunc, like (int) in the kernels
            sel = allowed & (lod < 0)
            for k in range(3):
                sel &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
            if not sel.any():
                continue
            rz, ry, rx = r["density"].shape
            ext = (rx, ry, rz)
            density = np.asarray(r["density"])
            label[sel] = np.asarray(r["labels"])[ic[2][sel] % rz, ic[1][sel] % ry, ic[0][sel] % rx].astype(np.uint32)
            lod[sel] = n
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


# ---- the three lookups of the reused twins, with the linear sample in place of the nearest texel
def _slab_lookup(rings, dx, inside):
    value, label, lod = linear_sample(rings, dx, inside)
    return value, label, np.where(lod < 0, 255, lod).astype(np.uint8)


def _composite_lookup(rings, size, coord):
    value, label, lod = linear_sample(rings, [coord[k] * size[k] for k in range(3)])
    return value, label, lod >= 0


def _iso_lookup(rings, size, coord=None, data=None):
    return linear_sample(rings, [coord[k] * size[k] for k in range(3)] if data is None else data)


@contextlib.contextmanager
def _sampling(module, lookup):
    saved = module.lookup
    module.lookup = lookup
    try:
        yield
    finally:
        module.lookup = saved


def slab_linear(*args, **kwargs):
    """slab_twin.slab_twin with every value_k the linear sample."""
    with _sampling(slab_twin, _slab_lookup):
        return slab_twin.slab_twin(*args, **kwargs)


def composite_linear(*args, **kwargs):
    """composite_twin.composite_twin with s of every sample the linear sample (labels stay the nearest sample's)."""
    with _sampling(composite_twin, _composite_lookup):
        return composite_twin.composite_twin(*args, **kwargs)


def iso_linear(*args, **kwargs):
    """iso_twin.iso_twin with S(iter) and D(p) the linear sample."""
    with _sampling(iso_twin, _iso_lookup):
        return iso_twin.iso_twin(*args, **kwargs)


def slice_linear(rings, world_inv, size, origin, u, v, width, height, material, colorspace_srgb=True, region=None):
    """svr_slice under SVR_INTERP_LINEAR; arguments and result as ``slice_twin.slice_twin``."""
    with np.errstate(all="ignore"):
        m = np.asarray(world_inv, f32).reshape(4, 4)
        size = [f32(s) for s in size]
        o, u, v = [f32(c) for c in origin], [f32(c) for c in u], [f32(c) for c in v]
        x, y = frame_pixels(width, height, region)
        in_frame = (x < width) & (y < height)
        fx = (x.astype(f32) + f32(0.5)) - f32(0.5) * f32(width)
        fy = (y.astype(f32) + f32(0.5)) - f32(0.5) * f32(height)
        p = [(o[k] + fx * u[k]) + fy * v[k] for k in range(3)]
        q = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] * f32(1.0) for k in range(3)]
        dx = [((q[k] + f32(0.5)) / size[k]) * size[k] for k in range(3)]
        inside = in_frame.copy()
        for k in range(3):
            inside &= (dx[k] >= 0) & (dx[k] < size[k])
        value, label, lod = _slab_lookup(rings, dx, inside)
        hit = lod != 255
        shape = x.shape
        flags = np.where(hit, HIT, np.where(inside, MISS, DISCARD)).astype(np.uint8)
        rgba = np.zeros(shape + (4,), f32)
        rgba[inside & ~hit] = (0, 0, 0, 1)
        if hit.any():
            mat = material
            s = (value[hit] - f32(mat["clim"][0])) / (f32(mat["clim"][1]) - f32(mat["clim"][0]))
            if f32(mat["gamma"]) != f32(1.0):
                s = np.power(s, f32(mat["gamma"]), dtype=f32)
            if colorspace_srgb:
                s = np.where(s <= f32(0.04045), s / f32(12.92), np.power((s + f32(0.055)) / f32(1.055), f32(2.4), dtype=f32))
            colors = np.asarray(mat["colors"], f32)
            hs = colors[label[hit] % np.uint32(len(colors))]
            rgb = hsv_to_rgb(hs[:, 0], hs[:, 1], s.astype(f32))
            rgba[hit] = np.stack([*rgb, np.full_like(rgb[0], f32(mat["opacity"]))], axis=-1)
        return dict(rgba=rgba, depth=np.zeros(shape, f32), label=label, flags=flags, value=value, lod=lod)


# ---- for a SceneSpec's volume after its ``center_on_position`` calls (the shapes of the other twins' twin_of_spec)
def _rings_of(spec, vol, rings):
    vol = vol or lmip.oracle_volume(spec)
    return vol, (lmip.rings_of(vol) if rings is None else rings)


def slice_of_spec(spec, origin, u, v, width, height, *, world_inv=None, region=None, vol=None, rings=None):
    vol, rings = _rings_of(spec, vol, rings)
    return slice_linear(rings, spec.world().inverse_matrix if world_inv is None else world_inv,
                        vol.volume_dimensions_shader, origin, u, v, width, height, material_of(spec.material),
                        colorspace_srgb=(spec.colorspace == "srgb"), region=region)


def slab_of_spec(spec, origin, u, v, w, samples, mode, width, height, *, world_inv=None, region=None, vol=None,
                 rings=None):
    vol, rings = _rings_of(spec, vol, rings)
    return slab_linear(rings, spec.world().inverse_matrix if world_inv is None else world_inv,
                       vol.volume_dimensions_shader, origin, u, v, w, samples, mode, width, height,
                       material_of(spec.material), colorspace_srgb=(spec.colorspace == "srgb"), region=region)
