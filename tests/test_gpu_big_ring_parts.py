"""GPU: density rings of 4 GiB or more at every kind of part split (csrc/ring_parts.h).  The march reaches such a ring
through up to 8 buffer resources of `zsplit` whole ring z planes each; these scenes put the level-0 window across the
part boundaries of splits of 3 and 2 planes (planes of 1 to 1.6 GiB, with a micro-block copy whose blocks a split of 3
float planes or of 2 uint16 planes would cut, and one whose blocks a split of 2 float planes does not), of 8 parts (the
span kernel's ceiling) and of 9 parts (the straightforward kernel's 64-bit addressing).  Every frame comes from both
code objects of the march and equals the oracle's on a small ring that holds the same window.  Each test holds one
volume at a time, at most about 18 GB of device memory.

Ring extents stay below 2^15 on every axis: beyond that the span kernel runs no direct batches (MarchParams::lod_pow2),
and only direct batches gather from the copy or switch resources per batch."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lmip
from slab_twin import twin_of_spec as slab_twin_of_spec
from slice_twin import twin_of_spec as slice_twin_of_spec
from sub_volume_renderer_amd import SubVolume, _native as N, synth, testing
from test_gpu_slab import check as check_slab
from test_gpu_slice import check as check_slice

pytestmark = pytest.mark.gpu
RGBA_TOL = 1e-4
# from outside the volume, 170 units from the target
VIEWS = ((-0.80, 0.36, 0.48), (0.05, 0.08, -1.0), (0.6, -0.3, 0.74))
# (eye, direction) from inside a level-0 window 4 planes thick (z 28 .. 31): the direct batches of the span kernel, and
# with them the micro-block copy, need runs of 8 samples that every lane of a wave takes on one LOD, which only rays
# that graze the window give.  Rays go up and down through the window's planes, across the part boundary
INSIDE_VIEWS = (((4.0, 6.0, 30.4), (0.8, 0.6, 0.05)), ((60.0, 8.0, 29.8), (-0.7, 0.7, -0.08)),
                ((32.0, 52.0, 30.9), (0.3, -0.95, 0.12)))
# LOD 1: a 64^3 ring over the whole 32^3 level, no micro-block copy (so that the copy census is LOD 0's alone)
LOD1_CHUNK, LOD1_RING, LOD1_SIZE = (4, 4, 16), (16, 16, 4), (32, 32, 32)


def _assert_frame(res, ref, what):
    """`res`: the (production, instrumented) pair of `testing.render_both`."""
    for r in res:
        rep = testing.compare(r, ref)
        assert rep["flags_equal"] and rep["labels_equal"] and rep.get("steps_equal", True), (what, rep)
        assert rep["rgba_max_rel"] <= RGBA_TOL and rep["depth_max_abs"] <= 1e-4, (what, rep)


def _specs(storage, lod0_chunk, lod0_ring, lod0_small, lod0_size, target, twin):
    """(big, small): the same label-less two-LOD scene with the level-0 ring `lod0_ring` chunks (numpy order) and with a
    small one, `lod0_small` chunks, that holds the same window.  `storage`: "uint8", "uint16" or "float32"."""
    pairs = []
    for k in range(2):
        d, _ = synth.volume(64, k)
        pairs.append((d.astype(np.uint16) * np.uint16(200) if storage == "uint16" else d, None))
    kw = dict(threshold=0.45, pairs=pairs, chunk_shapes=[lod0_chunk, LOD1_CHUNK])
    big = testing.synthetic_spec(64, 160, 96, ring_shapes=[lod0_ring, LOD1_RING], **kw)
    small = testing.synthetic_spec(64, 160, 96, ring_shapes=[lod0_small, LOD1_RING], **kw)
    for s in (big, small):
        if storage == "uint16":
            s.material.update(lmip_threshold=0.45 * 51000, clim=(0.0, 51000.0))
        s.ring_storage = "float32" if storage == "float32" else "native"
        s.centers = [(tuple(target), [lod0_size, LOD1_SIZE])]
        s.depth_range = (0.2, 4000.0)
    big.blocked_twin = [1 if twin else 0, 0]       # asked for explicitly: "auto" gives the copy up when HBM runs short
    return big, small


@contextlib.contextmanager
def _scene(spec, storage, ring_xyz, roi_begin_z, twin):
    scene = testing.build(spec)
    try:
        rings = scene.volume._rings
        assert rings.density_storage == storage
        assert tuple(scene.volume.wrapping_buffers[0].shape_in_pixels)[::-1] == ring_xyz
        assert rings.blocked_twin == [1 if twin else 0, 0]
        assert scene.volume.wrapping_buffers[0]._current_logical_roi_in_pixels.begin[0] == roi_begin_z
        yield scene
    finally:
        scene.volume.close()


def _views(big, small, target):
    for view in VIEWS:
        dvec = np.array(view) / np.linalg.norm(view)
        for s in (big, small):
            s.cam_position, s.cam_target = tuple(np.array(target) + 170.0 * dvec), tuple(target)
        yield view


def _inside_views(big, small):
    for eye, d in INSIDE_VIEWS:
        for s in (big, small):
            s.cam_position, s.cam_target = eye, tuple(np.array(eye) + 10.0 * np.array(d))
        yield eye, d


def _census(vol):
    census = (C.c_uint32 * 8)()
    N.check(N.lib().svr_debug_counters(vol._rings.handle, census, 1), "svr_debug_counters")
    return list(census)


def _copy_gathers(vol):
    timers = (C.c_uint64 * 16)()
    N.check(N.lib().svr_debug_timers(vol._rings.handle, timers, 1), "svr_debug_timers")
    return int(timers[15])


def _set_variant(vol, variant):
    N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")


def _frames_with_the_copy(big, small, scene, what, *, modes=("lmip", "mip")):
    """Every inside view in every mode, rendered with variant 0 and with 0x200 (every wave that can is sent to the micro-block
    copy): each frame == the oracle's.  Returns the direct batches (census [1]) and the gathers from the copy
    (svr_debug_timers()[15]) of the 0x200 frames."""
    vol = scene.volume
    served = direct = 0
    for mode in modes:
        vol.material.render_mode = mode
        small.material = dict(small.material, render_mode=mode)
        for view in _inside_views(big, small):
            ref = lmip.render_spec(small)
            assert (ref.flags == 2).sum() > 5000, (what, mode, view)
            for variant in (0, 0x200):
                _set_variant(vol, variant)
                _copy_gathers(vol)
                res = testing.render_both(vol, big.camera(), big.width, big.height)
                gathers = _copy_gathers(vol)
                census = _census(vol)
                _assert_frame(res, ref, (what, mode, view, hex(variant), "copy gathers", gathers, "census", census))
                assert census[6] > 0, "the span kernel must run (the straightforward kernel keeps no census)"
                if variant == 0x200:
                    served, direct = served + gathers, direct + census[1]
            _set_variant(vol, 0)
    vol.material.render_mode = "lmip"
    small.material = dict(small.material, render_mode="lmip")
    return served, direct


def test_a_float_ring_of_1_gib_planes_cut_mid_block_reads_rows():
    """A. float32 ring (x, y, z) = (16384, 16384, 4): 4 GiB of 1 GiB planes, so parts of 3 planes + 1.  The copy keeps 2
    float planes per block: ring planes 2 and 3 share a block that starts at 2 GiB, across the part boundary at plane 3
    (3 GiB).  The march must read rows there (no gather from the copy), and the frames equal the oracle's.  Slices and
    slabs still read the copy (64-bit indices): from it they equal the restatement bit for bit."""
    target = (31.5, 31.5, 30.0)                      # level-0 window z 28 .. 31 = ring planes 0 .. 3
    big, small = _specs("float32", (4, 8, 16), (1, 2048, 1024), (1, 8, 4), (4, 48, 48), target, twin=True)
    with _scene(big, "float32", (16384, 16384, 4), 28, twin=True) as scene:
        served, direct = _frames_with_the_copy(big, small, scene, "f32, parts of 3 planes")
        assert served == 0, f"{served} batches gathered from a copy whose blocks the part boundary cuts"
        assert direct > 0, "no direct batch ran: the copy was never in question"
        vol = scene.volume
        orac = lmip.oracle_volume(small)
        _set_variant(vol, 0x200)
        try:
            slices = [SubVolume.axis_slice_plane("z", (31.5, 31.5, 30.0), 0.5),     # ring plane 2: copy block 1, 2 GiB in
                      SubVolume.axis_slice_plane("z", (31.5, 31.5, 31.0), 0.5),     # ring plane 3: the second part
                      SubVolume.axis_slice_plane("x", (31.5, 31.5, 30.0), 0.5),     # across every plane
                      ((30.0, 33.0, 30.2), (0.6, 0.3, -0.05), (-0.1, 0.5, 0.06))]
            for pl in slices:
                res = vol.render_slice(*pl, big.width, big.height)
                torch.cuda.synchronize()
                ref = slice_twin_of_spec(small, *pl, big.width, big.height, vol=orac)
                check_slice(res, ref, ("f32 slice from the copy", pl))
                assert (ref["lod"] == 0).sum() > 800
            slabs = [(SubVolume.axis_slab_plane("z", (31.5, 31.5, 30.0), 0.5, 1.0), 4, "max"),
                     (SubVolume.axis_slab_plane("z", (31.5, 31.5, 30.0), 0.5, 0.5), 8, "mean"),
                     (SubVolume.axis_slab_plane("x", (31.5, 31.5, 30.0), 0.5, 1.0), 9, "min")]
            for sl, n, mode in slabs:
                res = vol.render_slab(*sl, n, big.width, big.height, mode=mode)
                torch.cuda.synchronize()
                ref = slab_twin_of_spec(small, *sl, n, mode, big.width, big.height, vol=orac)
                check_slab(res, ref, ("f32 slab from the copy", n, mode))
                assert (ref["lod"] == 0).sum() > 800
        finally:
            _set_variant(vol, 0)


def test_a_uint16_ring_of_1_5_gib_planes_cut_mid_block_reads_rows():
    """B. uint16 ring (28672, 28672, 4): 6.1 GiB of 1.53 GiB planes, parts of 2 planes.  The copy keeps 4 uint16 planes
    per block, which the boundary at plane 2 cuts in half: the march must read rows, and the frames equal the
    oracle's.  About 13 GB."""
    target = (31.5, 31.5, 30.0)
    big, small = _specs("uint16", (4, 8, 16), (1, 3584, 1792), (1, 8, 4), (4, 48, 48), target, twin=True)
    with _scene(big, "uint16", (28672, 28672, 4), 28, twin=True) as scene:
        served, direct = _frames_with_the_copy(big, small, scene, "u16, parts of 2 planes")
        assert served == 0, f"{served} batches gathered from a copy whose blocks the part boundary cuts"
        assert direct > 0, "no direct batch ran: the copy was never in question"


def test_a_float_ring_of_1_5_gib_planes_in_whole_blocks_gathers_from_the_copy():
    """C. float32 ring (20480, 20480, 4): 6.25 GiB of 1.56 GiB planes, parts of 2 planes = 1 block of the copy each.  With
    0x200 the copy serves gathers on both sides of the boundary at plane 2, and the frames equal the oracle's."""
    target = (31.5, 31.5, 30.0)
    big, small = _specs("float32", (4, 8, 16), (1, 2560, 1280), (1, 8, 4), (4, 48, 48), target, twin=True)
    with _scene(big, "float32", (20480, 20480, 4), 28, twin=True) as scene:
        served, _ = _frames_with_the_copy(big, small, scene, "f32, parts of 2 planes")
        assert served > 0, "no batch gathered from the micro-block copy"


def test_a_byte_ring_of_8_parts_stays_on_the_span_kernel():
    """D. uint8 ring (23168, 23176, 32): 16 GiB of planes just above 512 MiB, parts of 4 planes, 8 parts: the most the
    span kernel addresses.  The level-0 window holds ring planes 24 .. 31 and 0 .. 7, across the boundaries at planes 28
    and 4 and the ring's wrap; extents that are multiples of 8 keep empty-space skipping on.  LMIP and MIP."""
    target = (31.5, 31.5, 32.0)                      # level-0 window z 24 .. 39
    big, small = _specs("uint8", (8, 8, 16), (4, 2897, 1448), (2, 8, 4), (16, 48, 48), target, twin=False)
    with _scene(big, "uint8", (23168, 23176, 32), 24, twin=False) as scene:
        direct = 0
        vol = scene.volume
        for mode in ("lmip", "mip"):
            vol.material.render_mode = mode
            small.material = dict(small.material, render_mode=mode)
            for view in _views(big, small, target):
                ref = lmip.render_spec(small)
                assert (ref.flags == 2).sum() > 200, (mode, view)
                res = testing.render_both(vol, big.camera(), big.width, big.height)
                census = _census(vol)
                _assert_frame(res, ref, ("u8, 8 parts", mode, view))
                assert census[6] > 0, ("the span kernel must run (the straightforward kernel keeps no census)", census)
                direct += census[1]
        assert direct > 0, "no direct batch ran"


def test_a_byte_ring_of_9_parts_takes_the_straightforward_kernel():
    """E. uint8 ring (23168, 23176, 33): 16.5 GiB of planes just above 512 MiB, 9 parts of 4 planes, one more than the span kernel
    addresses: every draw takes the straightforward kernel's 64-bit addressing (no census), and the level-0 window
    (ring planes 22 .. 32 and 0 .. 10: 11 to 16.5 GiB into the ring, and across its wrap) equals the oracle's in LMIP
    and in the weighted average (march_wavg)."""
    target = (31.5, 31.5, 33.0)                      # level-0 window z 22 .. 43
    big, small = _specs("uint8", (11, 8, 16), (3, 2897, 1448), (2, 8, 4), (22, 48, 48), target, twin=False)
    with _scene(big, "uint8", (23168, 23176, 33), 22, twin=False) as scene:
        vol = scene.volume
        for mode in ("lmip", "weighted_average"):
            vol.material.render_mode = mode
            small.material = dict(small.material, render_mode=mode)
            if mode == "weighted_average":
                vol.material.weight_falloff = 0.5
                small.material["weight_falloff"] = 0.5
            for view in _views(big, small, target):
                ref = lmip.render_spec(small)
                assert (ref.flags == 2).sum() > 200, (mode, view)
                res = testing.render_both(vol, big.camera(), big.width, big.height)
                census = _census(vol)
                _assert_frame(res, ref, ("u8, 9 parts", mode, view))
                assert census[6] == 0, ("the span kernel ran on a ring it cannot address", census)
