"""GPU: the march's separable address into the micro-block copy of a ring (csrc/twin_address.h).  Every wave is routed to
the copy; frames must be the oracle's and, bit for bit, those of the same volume without a copy — on a ring whose
window wraps on all three axes at once (lanes past a wrap carry negative constants), for the three ring storages, in
LMIP, full-length and MIP marches (MIP: every sample of a ray counts, so every address does); and on a pair of rings on
either side of the predicate that routes a ring to the separable form (svr_twin_separable: 16-bit weights)."""
import numpy as np
import pytest

from oracle import lmip
from sub_volume_renderer_amd import _native as N, testing

from test_gpu_render import check
from test_gpu_twin import ALWAYS, twin_batches

pytestmark = pytest.mark.gpu

SHAPE = (96, 80, 160)                     # (z, y, x), the volume of test_micro_block_copy_follows_the_ring_through_wrapped_loads
CHUNK, RING = (4, 4, 16), (6, 5, 4)       # a ring of 24 x 20 x 64 slots
# the default window (one chunk less than the ring: 20 x 16 x 48 voxels) centred here starts at voxel (40, 32, 112): past
# one whole ring on every axis (constants of -ring before the wrap, -2 ring after it) and it crosses a ring boundary on
# every axis (48, 40, 128)
CENTRE_XYZ = (136.0, 40.0, 50.0)
CAMERAS = {"oblique": (-0.80, 0.36, 0.48), "along_z": (0.0, 0.0, 1.0)}


def _material(top, mode):
    m = dict(lmip_threshold=float("inf") if mode == "full" else 0.97 * top, lmip_fall_off=0.5, lmip_max_samples=10,
             fog_density=0.01, fog_color=(0.5, 0.5, 0.5), colors=[(k / 4, 1.0, 1.0) for k in range(4)], clim=(0.0, top))
    if mode == "mip":
        m["render_mode"] = "mip"
    return m


def _volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    data = rng.integers(1, 255, shape).astype(dtype) * (257 if dtype == np.uint16 else 1)
    seg = rng.integers(0, 4096, shape, dtype=np.uint32)
    return data.astype(dtype), seg


@pytest.fixture(scope="module")
def volumes():
    return {dt: _volume(SHAPE, dt, 7) for dt in (np.uint8, np.uint16)}


def _frames_with_and_without_the_copy(spec, want_hits):
    ref = lmip.render_spec(spec)
    frames = {}
    for twin in (True, False):
        spec.blocked_twin = [twin]
        scene = testing.build(spec)
        assert scene.volume._rings.blocked_twin == [twin]
        N.check(N.lib().svr_set_variant(scene.volume.prepare(), ALWAYS), "svr_set_variant")
        twin_batches(scene.volume)
        frames[twin], _, _ = check(scene, ref=ref, want_hits=want_hits)
        used = twin_batches(scene.volume)
        assert (used > 0) == twin, (twin, used)            # the copy really served gathers, and only where it exists
    same = testing.planes_identical(frames[True], frames[False])
    assert same and all(same.values()), same


@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("storage,dtype", [("native", np.uint8), ("native", np.uint16), ("float32", np.uint8)],
                         ids=["u8rings", "u16rings", "f32rings"])
@pytest.mark.parametrize("mode", ["lmip", "full", "mip"])
def test_window_wrapped_on_three_axes_every_wave_on_the_copy(volumes, cam, storage, dtype, mode):
    top = 65535.0 if dtype == np.uint16 else 255.0
    d = np.array(CAMERAS[cam], float)
    centre = np.array(CENTRE_XYZ)
    spec = testing.SceneSpec(pairs=[volumes[dtype]], chunk_shapes=[CHUNK], ring_shapes=[RING], material=_material(top, mode),
                             width=128, height=128, cam_position=tuple(centre + 70.0 * d / np.linalg.norm(d)),
                             cam_target=tuple(centre), depth_range=(0.5, 1000.0), centers=[(CENTRE_XYZ, None)])
    spec.ring_storage = storage
    _frames_with_and_without_the_copy(spec, want_hits=mode != "full")


@pytest.fixture(scope="module")
def slab():
    return _volume((16, 520, 1040), np.uint8, 11)


@pytest.mark.parametrize("mode", ["lmip", "mip"])
@pytest.mark.parametrize("ring_y", [512, 516])
def test_ring_planes_on_either_side_of_the_predicate(slab, ring_y, mode):
    """Finest ring planes of 1024 x 512 slots (Wz = 65532: the separable form) and 1024 x 516 (the general one); the
    window is the whole ring and wraps along x and y."""
    chunk = (4, 8, 16) if ring_y == 512 else (4, 4, 16)
    ring = (4, ring_y // chunk[1], 64)
    size = (16, ring_y, 1024)
    offset = (0, chunk[1], 16)                                            # a chunk in: slots [offset, ring) and [0, offset)
    centre = tuple(float(o + s // 2) for o, s in zip(offset, size))[::-1]
    d = np.array((0.05, 0.03, 1.0))
    spec = testing.SceneSpec(pairs=[slab], chunk_shapes=[chunk], ring_shapes=[ring], material=_material(255.0, mode),
                             width=160, height=120, cam_position=tuple(np.array(centre) + 1300.0 * d / np.linalg.norm(d)),
                             cam_target=centre, depth_range=(1.0, 5000.0), centers=[(centre, [size])])
    ref = lmip.render_spec(spec)
    spec.blocked_twin = [True]
    scene = testing.build(spec)
    assert scene.volume._rings.blocked_twin == [True]
    buf = scene.volume.wrapping_buffers[0]
    assert tuple(int(v) for v in buf.shape_in_pixels) == size
    N.check(N.lib().svr_set_variant(scene.volume.prepare(), ALWAYS), "svr_set_variant")
    twin_batches(scene.volume)
    check(scene, ref=ref)
    assert twin_batches(scene.volume) > 0
