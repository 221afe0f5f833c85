"""GPU: the march's scaled-ray instantiation (march_span<..., SCALED = true>, DESIGN.md "Scaled ray").  Where every LOD's
size * scale is an exact power of two >= 1 (MarchParams::ss_pow2), a fast run keeps the ray multiplied by that factor and
evaluates each voxel coordinate in two IEEE operations instead of three.  The identity is exact by construction; these
scenes hold it to the oracle on every plane, next to volumes whose extents are not powers of two (the unscaled kernel):

- power-of-two volumes (64^3), one non-power-of-two axis (64 x 64 x 96 voxels, x y z) and none at all (60^3);
- perspective cameras outside and inside the volume, axis-aligned orthographic views (two step components exactly 0);
- full and LMIP mode; byte, uint16 and float32 rings; with and without the micro-block copy forced on every wave;
- 2 and 8 LODs."""
import functools

import numpy as np
import pytest

import ortho_scenes as ortho
from sub_volume_renderer_amd import _native as N, synth, testing

from test_gpu_render import check

pytestmark = pytest.mark.gpu

ALWAYS = 0x200          # svr_set_variant bit 9: every wave takes the micro-block copy / stages bricks


@functools.lru_cache(maxsize=None)
def _pairs(shape_zyx, nl=3):
    """LOD k of a synthetic volume of `shape_zyx` voxels: the first shape >> k voxels of a cube's LOD k."""
    n = 1 << int(np.ceil(np.log2(max(shape_zyx))))
    out = []
    for k in range(nl):
        d, l = synth.volume(n, k)
        z, y, x = (s >> k for s in shape_zyx)
        out.append((np.ascontiguousarray(d[:z, :y, :x]), np.ascontiguousarray(l[:z, :y, :x])))
    return tuple(out)


SHAPES = {"pow2": (64, 64, 64), "tall": (96, 64, 64), "odd": (60, 60, 60)}


def _spec(shape, camera, full, storage):
    pairs = list(_pairs(SHAPES[shape]))
    if storage == "uint16":
        pairs = [(d.astype(np.uint16) * 257, l) for d, l in pairs]
    spec = testing.synthetic_spec(64, 64, 64, inside=camera == "K2", full=full, pairs=pairs)
    if storage == "uint16" and not full:
        spec.material.update(lmip_threshold=0.5 * 65535, clim=(0.0, 65535.0))
    if storage == "float32":
        spec.ring_storage = "float32"
    size = np.array(SHAPES[shape][::-1], float)
    centre = tuple((size - 1) / 2)
    spec.centers = [(centre, None)]
    if camera.startswith("ortho"):
        ortho.axis_view(spec, camera[5:], ppv=1)
    return spec


@pytest.mark.parametrize("storage", ["native", "uint16", "float32"])
@pytest.mark.parametrize("full", [False, True], ids=["lmip", "full"])
@pytest.mark.parametrize("camera", ["K1", "K2", "ortho+x", "ortho-z"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_scaled_and_unscaled_chains_match_oracle(shape, camera, full, storage):
    scene = testing.build(_spec(shape, camera, full, storage))
    check(scene, want_hits=False)


@pytest.mark.parametrize("full", [False, True], ids=["lmip", "full"])
@pytest.mark.parametrize("camera", ["K1", "ortho-y"])
@pytest.mark.parametrize("shape", ["pow2", "tall"])
def test_micro_block_copy_on_every_wave(shape, camera, full):
    scene = testing.build(_spec(shape, camera, full, "native"))
    N.check(N.lib().svr_set_variant(scene.volume.prepare(), ALWAYS), "svr_set_variant")
    check(scene, want_hits=False)


@pytest.mark.parametrize("camera", ["K1", "K2", "ortho+z"])
@pytest.mark.parametrize("nl", [2, 8])
def test_two_and_eight_lods(nl, camera):
    n = 256 if nl == 8 else 64
    pairs = list(_pairs((n, n, n), nl))
    chunks = [tuple(min(8, n >> k) for _ in range(3)) for k in range(nl)]
    rings = [(4, 4, 3)] * nl
    spec = testing.synthetic_spec(n, 64, 64, inside=camera == "K2", pairs=pairs, chunk_shapes=chunks, ring_shapes=rings)
    if camera.startswith("ortho"):
        ortho.axis_view(spec, camera[5:], ppv=1)
    check(testing.build(spec), want_hits=False)


def test_tilted_orthographic_rays_with_tiny_step_components():
    """An orthographic view a hair off the x axis: the y and z step components are some 1e-7 of x's."""
    spec = _spec("pow2", "ortho+x", False, "native")
    pos = np.array(spec.cam_position)
    tgt = np.array(spec.cam_target) + np.array([0.0, 3e-7, -2e-7])
    spec.cam_target = tuple(float(v) for v in tgt)
    spec.cam_position = tuple(float(v) for v in pos)
    d = ortho.direction_column(spec)
    assert np.count_nonzero(d) == 3 and np.min(np.abs(d)) < 1e-5 * np.max(np.abs(d)), d
    check(testing.build(spec), want_hits=False)
