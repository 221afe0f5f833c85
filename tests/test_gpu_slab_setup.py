"""GPU: the set-up of a brick slab (march_kernel.hip, "LDS brick slabs"; csrc/slab_box.h): the wave's bounding box comes
from one reduction of packed 16-bit halves, and the box is staged into LDS chunk by chunk.  Every wave is made to stage
bricks (svr_set_variant bit 9) and no LOD keeps a micro-block copy, so LOD 0 stages them too.  Frames are held to the
oracle on every plane and on the step counts, and bit for bit to the same scene rendered without bricks (bit 8): a box
that missed a sample, or a row staged to the wrong place, shows as a wrong texel."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmip
from sub_volume_renderer_amd import FrameRegion, _native as N, synth, testing

pytestmark = pytest.mark.gpu

BRICKS = 0x200          # svr_set_variant bit 9: every wave stages bricks wherever a LOD allows it
NO_BRICKS = 0x100       # bit 8: linear gathers only
N_VOX = 96


def census(volume):
    """[2] brick batches, [3] brick slabs of the instrumented renders since the last call (svr_debug_counters)"""
    c = (C.c_uint32 * 8)()
    N.check(N.lib().svr_debug_counters(volume._rings.handle, c, 1), "svr_debug_counters")
    return list(c)


_PAIRS = {}


def pairs_of(dtype):
    if dtype not in _PAIRS:
        base = [synth.volume(N_VOX, k, 4096) for k in range(3)]
        _PAIRS[dtype] = base if dtype == "uint8" else [(d.astype(np.uint16) * 257, l) for d, l in base]
    return _PAIRS[dtype]


def make_spec(dtype, storage, mode, cam, w=203, h=131):
    """96^3, 3 LODs, rings 16-aligned in x; the LOD windows wrap around their rings on all three axes (re-centred twice);
    a frame of 203 x 131 pixels leaves the last tile column and row partly outside (dead lanes in those waves)."""
    n = N_VOX
    spec = testing.synthetic_spec(n, w, h, full=(mode == "full"), pairs=pairs_of(dtype),
                                  chunk_shapes=[(8, 8, 16), (4, 4, 16), (2, 2, 16)], ring_shapes=[(6, 5, 3), (10, 10, 3), (16, 16, 2)])
    spec.ring_storage = storage
    spec.blocked_twin = [False, False, False]
    if dtype == "uint16":
        spec.material.update(lmip_threshold=spec.material["lmip_threshold"] * 257.0, clim=(0.0, 65535.0))
    if mode == "mip":
        spec.material.update(render_mode="mip")
    spec.centers = [((40.0, 44.0, 52.0), None), ((57.0, 49.0, 43.0), None)]
    c = (n - 1) / 2.0
    centre = np.array([c, c, c])
    if cam == "+x":                                   # outside, looking along +x (a little off the axis)
        spec.cam_position, spec.cam_target = tuple(centre + np.array([-1.7 * n, 0.03 * n, 0.05 * n])), (c, c, c)
    elif cam == "oblique":
        d = np.array([-1.0, -0.9, -0.8])
        spec.cam_position, spec.cam_target = tuple(centre + 1.7 * n * d / np.linalg.norm(d)), (c, c, c)
    else:
        assert cam == "ortho"
        spec.projection, spec.ortho_size, spec.depth_range = "orthographic", (1.3 * n * w / h, 1.3 * n), (1.0, 6.0 * n)
        d = np.array([0.7, -0.4, 0.59])
        spec.cam_position, spec.cam_target = tuple(centre + 2.0 * n * d / np.linalg.norm(d)), (c, c, c)
    return spec


def hold_with_and_without_bricks(spec, region=None, variant=BRICKS, want_slabs=True):
    ref = lmip.render_spec(spec, region=region)
    scene = testing.build(spec)
    vol = scene.volume
    N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")
    census(vol)
    rep = testing.hold_both_to(ref, vol, scene.camera, spec.width, spec.height, region=region)
    c = census(vol)
    if want_slabs:
        assert c[3] > 0 and c[2] > 0, c                               # slabs were set up, batches served from them
    N.check(N.lib().svr_set_variant(vol.prepare(), (variant & ~BRICKS) | NO_BRICKS), "svr_set_variant")
    off = testing.hold_both_to(ref, vol, scene.camera, spec.width, spec.height, region=region)
    assert census(vol)[3] == 0
    for which in ("production", "instrumented"):
        same = testing.planes_identical(rep[which], off[which])
        assert same and all(same.values()), (which, same)
    assert bool((rep["instrumented"].steps == off["instrumented"].steps).all())
    return rep, c


@pytest.mark.parametrize("cam", ["+x", "oblique", "ortho"])
@pytest.mark.parametrize("mode", ["lmip", "full", "mip"])
@pytest.mark.parametrize("dtype,storage", [("uint8", "native"), ("uint16", "native"), ("uint8", "float32")],
                         ids=["u8rings", "u16rings", "f32rings"])
def test_wrapped_windows_and_partly_covered_tiles(dtype, storage, mode, cam):
    rep, _ = hold_with_and_without_bricks(make_spec(dtype, storage, mode, cam))
    assert rep["n_miss" if mode == "full" else "n_hit"] > 0


@pytest.mark.parametrize("mode", ["lmip", "full"])
def test_tiles_with_a_single_live_lane(mode):
    """Regions of one pixel: the wave that renders it has 63 lanes outside the frame, which carry the sentinel through
    the whole reduction; the pixel sits in a different lane of its tile each time (and so in every row of 16 lanes)."""
    spec = make_spec("uint8", "native", mode, "oblique")
    ref_full = lmip.render_spec(spec)
    scene = testing.build(spec)
    vol = scene.volume
    N.check(N.lib().svr_set_variant(vol.prepare(), BRICKS), "svr_set_variant")
    slabs = 0
    for k, (x, y) in enumerate([(96, 64), (101, 65), (98, 67), (103, 70), (97, 69), (100, 71), (102, 66), (99, 68)]):
        region = FrameRegion.tile(x, y, 1, 1)
        ref = lmip.render_spec(spec, region=region)
        assert np.array_equal(ref.flags, ref_full.flags[y:y + 1, x:x + 1])
        census(vol)
        testing.hold_both_to(ref, vol, scene.camera, spec.width, spec.height, region=region)
        slabs += census(vol)[3]
    assert slabs > 0


def rows_of_the_tiles(spec, tw, th):
    """For an orthographic view: per wave tile of tw x th pixels that lies inside the frame and the volume, a lower and an
    upper bound of ny, the rows of y a slab's box has.  All rays are parallel, so the y coordinates of a tile's samples at
    one iteration differ by what its near-plane points do: `span`; the box has at least floor(span) + 1 rows and, with
    the ray's own travel in y over a slab (`drift`), at most ceil(span + drift) + 1."""
    import ortho_scenes as ortho

    near, ray = ortho.pixel_rays(spec)
    size = ortho.size_xyz(spec)
    inside = np.all([(near[k] > 0.0) & (near[k] < size[k] - 1.0) for k in (1, 2)], axis=0)
    drift = 26.0 * float(np.max(np.abs(ray[1] / ray[0])))               # a slab of 32 iterations is under 26 voxels of x
    lo, hi = [], []
    for y0 in range(0, spec.height - th + 1, th):
        for x0 in range(0, spec.width - tw + 1, tw):
            if inside[y0:y0 + th, x0:x0 + tw].all():
                span = float(np.ptp(near[1][y0:y0 + th, x0:x0 + tw]))
                lo.append(int(np.floor(span)) + 1)
                hi.append(int(np.ceil(span + drift)) + 1)
    return lo, hi


@pytest.mark.parametrize("tile,tw,th", [(0x220, 2, 32), (0x230, 4, 16)], ids=["tile2x32", "tile4x16"])
def test_boxes_with_more_rows_than_one_chunk(tile, tw, th):
    """A volume of 64 x 136 x 32 voxels seen along +x by an orthographic camera at 1.25 voxels per pixel.  Every slab of
    LOD 0 is 32 iterations long here (asserted: 4 batches per slab), about 25.6 voxels of x, more than one 16-voxel group:
    its box spans 2 or 3 groups, the row pitch gp is 3 and one load instruction stages rows_per = 64 // 3 = 21 rows.
    With wave tiles of 2 x 32 pixels every box has 39 rows or more (computed here from the rays), so every slab is
    staged in two chunks; with tiles of 4 x 16 pixels no box has more than 21 and the same scene runs the loop once:
    the control."""
    dens, lab = synth.volume(136, 0, 4096)
    d1, l1 = synth.volume(136, 1, 4096)
    pairs = [(dens[:32, :136, :64].copy(), lab[:32, :136, :64].copy()), (d1[:16, :68, :32].copy(), l1[:16, :68, :32].copy())]
    w, h = 40, 112
    spec = testing.SceneSpec(
        pairs=pairs, chunk_shapes=[(8, 8, 16), (4, 4, 16)], ring_shapes=[(4, 17, 4), (4, 17, 2)],
        material=dict(lmip_threshold=float("inf"), lmip_fall_off=0.5, lmip_max_samples=10, fog_density=0.01, fog_color=(0.5, 0.5, 0.5),
                      colors=[(k / 4, 1.0, 1.0) for k in range(4)], clim=(0.0, 255.0)),
        width=w, height=h, centers=[((31.5, 67.5, 15.5), None)])
    spec.blocked_twin = [False, False]
    spec.projection, spec.ortho_size, spec.depth_range = "orthographic", (1.25 * w, 1.25 * h), (1.0, 400.0)
    spec.cam_position, spec.cam_target = (-100.0, 67.9, 15.7), (31.5, 67.5, 15.5)
    rep, c = hold_with_and_without_bricks(spec, variant=BRICKS | tile)
    assert rep["n_miss"] > 0 and c[2] == 4 * c[3] > 0               # every slab is the long one: 4 batches of 8 iterations
    # ... which travels more than one 16-voxel group in x (a ray crosses the 64 voxels of x in `steps` iterations)
    steps = rep["instrumented"].steps.cpu().numpy().astype(np.int64)
    assert 32 * 64.0 / steps.max() > 17.0, steps.max()
    lo, hi = rows_of_the_tiles(spec, tw, th)
    assert len(lo) >= 8
    rows_per = 64 // 3
    if tile == 0x220:
        assert min(lo) > rows_per, (min(lo), rows_per)              # every box of these tiles needs a second chunk
    else:
        assert max(hi) <= rows_per, (max(hi), rows_per)             # one chunk
