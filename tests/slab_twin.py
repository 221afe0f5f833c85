"""numpy float32 restatement of svr_slab (include/svr.h, "thick-slab projections"), in the operation order stated
there: svr_slice's plane chain up to q, N samples of the LOD cascade along w (nearest, or with ``linear`` the linear
sample) reduced by max, min or mean, svr_slice's grey shading - the shared pieces are tests/twin_common.py's."""
import numpy as np

from twin_common import data_points, flags_of, material_of, plane_points, rings_of_spec, sample, shade_grey

f32 = np.float32
MODES = ("max", "min", "mean")


def w_len_of(w):
    """|w| as the caller passes it: the float32 of the float64 norm of the float32 vector."""
    return f32(np.linalg.norm(np.array([f32(c) for c in w], np.float64)))


def slab_twin(rings, world_inv, size, origin, u, v, w, samples, mode, width, height, material, colorspace_srgb=True,
              region=None, linear=False):
    """``rings``: oracle.lmip.rings_of(...) (or dicts of the same keys); ``world_inv``: row-major 4x4 (cast to f32
    here); ``size``: volume_dimensions in shader order.  Returns dict(rgba, depth, label, flags, value, lod)."""
    assert mode in MODES and 1 <= samples <= 4096
    with np.errstate(all="ignore"):
        return _slab(rings, world_inv, size, origin, u, v, w, samples, mode, width, height, material, colorspace_srgb,
                     region, linear)


def _slab(rings, world_inv, size, origin, u, v, w, N, mode, W, H, mat, srgb, region, linear):
    m, size, q, in_frame = plane_points(world_inv, size, origin, u, v, W, H, region)
    w = [f32(c) for c in w]
    dw = [(m[k, 0] * w[0] + m[k, 1] * w[1]) + m[k, 2] * w[2] for k in range(3)]
    half = f32(0.5) * f32(N - 1)

    shape = in_frame.shape
    hits = np.zeros(shape, np.int64)
    total = np.zeros(shape, f32)
    best = np.zeros(shape, f32)
    best_k = np.zeros(shape, np.int64)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, -1, np.int32)
    inside_any = np.zeros(shape, bool)
    for k in range(N):
        t = f32(k) - half
        dx, inside = data_points([q[i] + t * dw[i] for i in range(3)], size, in_frame)
        val, lab, lo = sample(rings, dx, inside, linear)
        hit = lo >= 0
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
    return dict(rgba=shade_grey(value, label, hit, inside_any, mat, srgb), depth=depth,
                label=np.where(hit, label, 0).astype(np.uint32), flags=flags_of(hit, inside_any), value=value,
                lod=np.where(hit, lod, 255).astype(np.uint8))


def twin_of_spec(spec, origin, u, v, w, samples, mode, width, height, *, world_inv=None, region=None, vol=None,
                 rings=None, linear=False):
    """The restatement for a SceneSpec's volume after its ``center_on_position`` calls."""
    vol, rings = rings_of_spec(spec, vol, rings)
    return slab_twin(rings, spec.world().inverse_matrix if world_inv is None else world_inv,
                     vol.volume_dimensions_shader, origin, u, v, w, samples, mode, width, height,
                     material_of(spec.material), colorspace_srgb=(spec.colorspace == "srgb"), region=region, linear=linear)
