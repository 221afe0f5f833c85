"""GPU: the control code around the march's batches (march_kernel.hip, `lmip_batch` and the loops that call it; DESIGN.md,
"Batch control").  Which lanes are live, which have found their first hit and which have left the loop travel as
wave-level lane masks; a wrong mask shows where the lanes of one wave differ: rays that end at every position inside a
batch, first hits on the first and on the last sample of a batch beside lanes that found nothing and lanes that are done,
and the materials that take the state machine's other forks.  A 64^3 synthetic scene at 96 x 64 through
`testing.hold_both_to`: both code objects of the march against the oracle on every plane and on the step counts, with
bricks forced on, forced off and probed, on byte (with and without the micro-block copy), uint16 and float32 rings."""
import ctypes as C

import numpy as np
import pytest

from oracle import lmip
from sub_volume_renderer_amd import _native as N, synth, testing

pytestmark = pytest.mark.gpu

N_VOX, W, H = 64, 96, 64
U = 8                                   # samples per batch of the march
INT32_MAX = 2**31 - 1
ROUTES = {"bricks": 0x200, "rows": 0x100, "probe": 0}      # svr_set_variant bits 9 / 8 / neither
# name -> (source dtype, ring storage, micro-block copy, factor of the stored values over the byte scene's)
RINGS = {"u8": ("uint8", "native", "auto", 1), "u8nocopy": ("uint8", "native", [False] * 3, 1),
         "u16": ("uint16", "native", "auto", 257), "f32": ("uint8", "float32", "auto", 1)}

_BASE = [synth.volume(N_VOX, k, 4096) for k in range(3)]
_SCENES, _ORACLE_VOLS, _REFS = {}, {}, {}


def spec_of(rings, distance=1.6):
    dtype, storage, twin, scale = RINGS[rings]
    pairs = _BASE if dtype == "uint8" else [(d.astype(np.uint16) * 257, l) for d, l in _BASE]
    spec = testing.synthetic_spec(N_VOX, W, H, pairs=pairs)
    spec.ring_storage, spec.blocked_twin = storage, twin
    spec.material.update(clim=(0.0, 255.0 * scale))
    c = (N_VOX - 1) / 2.0
    d = np.array([-0.80, 0.36, 0.48])
    spec.cam_position = tuple(np.array([c, c, c]) + distance * N_VOX * d / np.linalg.norm(d))
    return spec


def reference(rings, material, distance=1.6):
    """The oracle's frame of one case; float32 rings of byte sources hold the byte scene's values: one frame serves both.
    Computed once per case and left alone."""
    dtype, _, _, scale = RINGS[rings]
    key = (dtype, distance, tuple(sorted((k, repr(v)) for k, v in material.items())))
    if key not in _REFS:
        spec = spec_of("u8" if dtype == "uint8" else "u16", distance)
        spec.material.update(material)
        if dtype not in _ORACLE_VOLS:
            _ORACLE_VOLS[dtype] = lmip.oracle_volume(spec)
        _REFS[key] = lmip.render_spec(spec, vol=_ORACLE_VOLS[dtype])
    return _REFS[key]


def hold(rings, route, material, distance=1.6):
    """Both kernels against the oracle, on the scene of `rings` (built once) with this material, routing and camera"""
    scale = RINGS[rings][3]
    material = dict(material)
    if "lmip_threshold" in material:
        material["lmip_threshold"] = material["lmip_threshold"] * scale
    ref = reference(rings, material, distance)
    if rings not in _SCENES:
        _SCENES[rings] = testing.build(spec_of(rings))
    vol = _SCENES[rings].volume
    base = dict(lmip_fall_off=0.5, lmip_max_samples=10, render_mode="lmip")
    base.update(material)
    for k, v in base.items():
        setattr(vol.material, k, v)
    N.check(N.lib().svr_set_variant(vol.prepare(), ROUTES[route]), "svr_set_variant")
    rep = testing.hold_both_to(ref, vol, spec_of(rings, distance).camera(), W, H)
    return ref, rep


def tiles(*planes):
    """the 8 x 8 pixel tiles of a frame (one wave each), as tuples of 64-element arrays"""
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            yield tuple(p[y:y + 8, x:x + 8].reshape(-1).astype(np.int64) for p in planes)


# ---- ray ends
def ray_end_distance():
    """The first camera distance at which the rays of the frame end at all eight positions inside a batch (in full mode
    every ray runs to its end: the step plane holds nsteps)"""
    for distance in (1.6, 1.65, 1.7, 1.75, 1.8):
        ref = reference("u8", dict(lmip_threshold=float("inf")), distance)
        if len(np.unique(ref.steps[ref.flags == 1] % U)) == U:
            return distance
    return None


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("rings", RINGS)
def test_rays_that_end_at_every_position_of_a_batch(rings, route):
    distance = ray_end_distance()
    assert distance is not None
    ref, rep = hold(rings, route, dict(lmip_threshold=float("inf")), distance)
    ends = ref.steps[ref.flags == 1] % U
    assert sorted(np.unique(ends)) == list(range(U)), np.unique(ends)
    # ... and inside single waves: some tile alone holds at least four of them
    assert max(len(np.unique(s[f == 1] % U)) for f, s in tiles(ref.flags, ref.steps)) >= 4
    assert rep["n_miss"] > 1000


# ---- thresholds
def kinds_in_one_tile(ref, nsteps):
    """With lmip_max_samples = 1 a ray whose first hit is sample i executes i + 2 iterations (the hit, then the one that
    ends it) unless it ends there.  True if some tile holds, for one batch [b, b + 8): a lane whose first hit is sample b,
    or one whose first hit is sample b + 7 (`which` says), a lane that has found nothing by then and goes on beyond the batch
    (a miss whose ray is longer), and a lane that finished before b."""
    found = {"first": False, "last": False}
    for f, s, n in tiles(ref.flags, ref.steps, nsteps):
        hit, miss = f == 2, f == 1
        broke = hit & (s < n)
        first_i = s - 2
        for which, pos in (("first", 0), ("last", U - 1)):
            for b in np.unique((first_i[broke & (first_i % U == pos)] // U) * U):
                if (miss & (n > b + U)).any() and (broke & (s <= b)).any():
                    found[which] = True
    return found["first"] and found["last"]


def kinds_threshold():
    nsteps = reference("u8", dict(lmip_threshold=float("inf"))).steps
    for thr in range(24, 232, 4):
        ref = reference("u8", dict(lmip_threshold=float(thr), lmip_max_samples=1))
        if kinds_in_one_tile(ref, nsteps):
            return float(thr), nsteps
    return None, nsteps


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("rings", RINGS)
def test_first_hits_on_the_first_and_last_sample_of_a_batch(rings, route):
    thr, nsteps = kinds_threshold()
    assert thr is not None
    ref, rep = hold(rings, route, dict(lmip_threshold=thr, lmip_max_samples=1))
    assert kinds_in_one_tile(ref, nsteps)          # (uint16 rings hold 257 times the bytes: the same frame, asserted again)
    assert rep["n_hit"] > 0 and rep["n_miss"] > 0


# ---- state machines
MACHINES = {
    "mip_fork": dict(lmip_threshold=127.5, lmip_fall_off=0.0, lmip_max_samples=INT32_MAX),   # never stops: the MIP-like pre-check
    "one_sample": dict(lmip_threshold=127.5, lmip_max_samples=1),
    "thr_inf": dict(lmip_threshold=float("inf")),
    "thr_zero": dict(lmip_threshold=0.0),                     # every ray hits on its first sample
    "thr_above": dict(lmip_threshold=256.0),                  # above the largest stored value (x 257 on uint16 rings)
}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("rings", RINGS)
@pytest.mark.parametrize("machine", MACHINES)
def test_state_machine_forks(machine, rings, route):
    ref, rep = hold(rings, route, MACHINES[machine])
    if machine in ("thr_inf", "thr_above"):
        assert rep["n_hit"] == 0 and rep["n_miss"] > 1000
    elif machine == "thr_zero":
        assert rep["n_miss"] == 0 and rep["n_hit"] > 1000
    else:
        assert rep["n_hit"] > 100 and rep["n_miss"] > 100
    if machine == "mip_fork":                                  # a ray that hit runs to its end
        nsteps = reference(rings, dict(lmip_threshold=float("inf"))).steps
        assert np.array_equal(ref.steps[ref.flags == 2], nsteps[ref.flags == 2])


# ---- empty-space skipping
def test_skipping_with_lanes_that_follow_a_maximum_beside_lanes_that_veto():
    """An LMIP frame of sparse bright blobs in which waves skip empty space (census), with hits that are followed for 40 samples: some tile
    holds lanes that follow their maximum for many samples while others, still searching, pass occupied cells."""
    from test_gpu_skip import _scene, _sparse_pairs

    spec = _scene(128, _sparse_pairs(128, 2, count=300), 150.0, "K1")
    spec.material.update(lmip_fall_off=0.0, lmip_max_samples=40)         # a hit is followed for 40 samples, whatever they hold
    ref = lmip.render_spec(spec)
    scene = testing.build(spec)
    vol = scene.volume
    census = (C.c_uint32 * 8)()
    vol.prepare()
    N.check(N.lib().svr_debug_counters(vol._rings.handle, census, 1), "svr_debug_counters")
    testing.hold_both_to(ref, vol, scene.camera, spec.width, spec.height)
    N.check(N.lib().svr_debug_counters(vol._rings.handle, census, 1), "svr_debug_counters")
    assert census[7] > 0, list(census)                          # batches skipped as empty space
    mixed = 0
    for y in range(0, spec.height, 8):
        for x in range(0, spec.width, 8):
            f = ref.flags[y:y + 8, x:x + 8].reshape(-1)
            s = ref.steps[y:y + 8, x:x + 8].reshape(-1).astype(np.int64)
            hit = f == 2
            # hits that end 16 or more iterations apart: one lane followed its maximum while the other still searched
            if hit.sum() >= 2 and (f == 1).any() and np.ptp(s[hit]) >= 2 * U:
                mixed += 1
    assert mixed > 0
