"""tools/timing.py on the GPU: the two timers issue exactly the calls the tools/*_time.py scripts count on (--trace-db
attributes a traced run's dispatches by that count; no duration is asserted), and the structs `Outputs.of` /
`SliceOutputs.of` build drive svr_render / svr_slice to the planes SubVolume.render / render_slice give."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from helpers import assert_same_bits, fixture_arrays
from sub_volume_renderer_amd import SubVolume, _native as N, testing

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import timing  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 64, 48


class Counting:
    """One tiny torch op per call, counted."""

    def __init__(self):
        import torch

        self.calls = 0
        self.t = torch.zeros(64, device="cuda")

    def __call__(self):
        self.calls += 1
        self.t.add_(1.0)


def test_held_issues_warmup_plus_two_windows_per_box():
    one = Counting()
    call_s, gpu_s = timing.held(one, calls=3, boxes=2, warmup=4)
    assert one.calls == 4 + 2 * 2 * 3
    assert float(one.t[0]) == one.calls                       # every call ran, in stream order behind the held windows
    for box in (call_s, gpu_s):
        assert len(box) == 2 and all(math.isfinite(t) and t > 0 for t in box)
    again = Counting()
    timing.held(again, calls=2, boxes=3, warmup=0)            # the sleep probe is taken once per process
    assert again.calls == 2 * 3 * 2


def test_timed_issues_warmup_first_run_and_repeats():
    one = Counting()
    median, lo, hi, k = timing.timed(one, window_s=0.002, repeats=3, k0=2)
    assert k >= 2 and one.calls == 2 * 2 + 3 * k
    assert 0 < lo <= median <= hi and math.isfinite(hi)
    other = Counting()
    _, _, _, k = timing.timed(other, window_s=0.002, repeats=1, k0=4, warmup=3)     # outline_time.py's shape
    assert other.calls == 3 + 4 + k


@pytest.fixture(scope="module")
def scene():
    """The smallest ring fixture of helpers.py (16^3 uint16, 2^3 chunks of 4^3 resident) as a one-LOD volume seen from
    outside along -z: the rays through the middle of the frame meet voxels above the threshold."""
    data, seg, ring_chunks, chunk = fixture_arrays("F2")
    spec = testing.SceneSpec(pairs=[(data, seg)], chunk_shapes=[chunk], ring_shapes=[ring_chunks],
                             material=dict(lmip_threshold=1500.0, clim=(0.0, 4095.0)), width=W, height=H,
                             cam_position=(8.0, 8.0, 40.0), cam_target=(8.0, 8.0, 8.0), centers=[((8.0, 8.0, 8.0), None)])
    built = testing.build(spec)
    yield built
    built.volume.close()


def _host(res, names):
    return {n: getattr(res, n).cpu().numpy().copy() for n in names}


def _poison(res, names):
    for n in names:
        getattr(res, n).fill_(93)


def test_outputs_of_drives_svr_render_to_the_planes_of_render(scene):
    import torch

    vol, cam = scene.volume, scene.camera
    names = ("rgba", "depth", "label", "flags")
    res = vol.render(cam, W, H)
    torch.cuda.synchronize()
    want = _host(res, names)
    assert int((want["flags"] == N.SVR_PIX_HIT).sum()) > 0 and int((want["flags"] != N.SVR_PIX_HIT).sum()) > 0
    _poison(res, names)
    handle = vol.prepare()
    cb, fb = vol.camera_block(cam), vol.frame_block(W, H, None)
    ob = N.Outputs.of(res, pick_id=vol.id & 0xFFFFFFFF)
    stream = torch.cuda.current_stream().cuda_stream
    N.check(N.lib().svr_render(handle, C.byref(cb), C.byref(fb), C.byref(ob), C.c_void_p(stream)), "svr_render")
    torch.cuda.synchronize()
    got = _host(res, names)
    for n in names:
        assert_same_bits(got[n], want[n], n)


def test_slice_outputs_of_drives_svr_slice_to_the_planes_of_render_slice(scene):
    import torch

    vol = scene.volume
    names = ("rgba", "depth", "label", "flags", "value", "lod")
    origin, u, v = SubVolume.axis_slice_plane("z", (8.0, 8.0, 8.0), 0.25)
    res = vol.render_slice(origin, u, v, W, H)
    torch.cuda.synchronize()
    want = _host(res, names)
    assert int((want["flags"] == N.SVR_PIX_HIT).sum()) > 0 and np.unique(want["value"]).size > 4
    _poison(res, names)
    handle = vol.prepare()
    pl, fb = vol._plane_struct(origin, u, v), vol.frame_block(W, H, None)
    ob = N.SliceOutputs.of(res)
    stream = torch.cuda.current_stream().cuda_stream
    N.check(N.lib().svr_slice(handle, C.byref(pl), C.byref(fb), C.byref(ob), C.c_void_p(stream)), "svr_slice")
    torch.cuda.synchronize()
    got = _host(res, names)
    for n in names:
        assert_same_bits(got[n], want[n], n)
