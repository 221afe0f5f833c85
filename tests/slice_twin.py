"""numpy float32 restatement of svr_slice (include/svr.h, "cross-section views"), in the operation order stated
there: the plane chain, one sample of the LOD cascade (nearest, or with ``linear`` the linear sample), the grey
shading - each a piece of tests/twin_common.py."""
import numpy as np

from twin_common import (DISCARD, HIT, MISS, data_points, flags_of, material_of, plane_points,  # noqa: F401  (re-exported)
                         rings_of_spec, sample, shade_grey)

f32 = np.float32


def slice_twin(rings, world_inv, size, origin, u, v, width, height, material, colorspace_srgb=True, region=None,
               linear=False):
    """``rings``: oracle.lmip.rings_of(...) (shader-order offset / shape / scale, textures [z][y][x]);
    ``world_inv``: row-major 4x4 (cast to f32 here); ``size``: volume_dimensions in shader order.
    Returns dict(rgba, depth, label, flags, value, lod) for the output pixels of ``region`` (default: the frame)."""
    with np.errstate(all="ignore"):
        _, size, q, in_frame = plane_points(world_inv, size, origin, u, v, width, height, region)
        dx, inside = data_points(q, size, in_frame)
        value, label, lod = sample(rings, dx, inside, linear)
        hit = lod >= 0
        return dict(rgba=shade_grey(value, label, hit, inside, material, colorspace_srgb), depth=np.zeros(hit.shape, f32),
                    label=label, flags=flags_of(hit, inside), value=value,
                    lod=np.where(hit, lod, 255).astype(np.uint8))


def twin_of_spec(spec, origin, u, v, width, height, *, world_inv=None, region=None, vol=None, rings=None, linear=False):
    """The restatement for a SceneSpec's volume after its ``center_on_position`` calls."""
    vol, rings = rings_of_spec(spec, vol, rings)
    return slice_twin(rings, spec.world().inverse_matrix if world_inv is None else world_inv,
                      vol.volume_dimensions_shader, origin, u, v, width, height, material_of(spec.material),
                      colorspace_srgb=(spec.colorspace == "srgb"), region=region, linear=linear)
