"""GPU: a composite render still in flight is never overwritten under it.  Its stream is held by a bounded sleep kernel,
so the composite runs only well after the host has enqueued a blocking ring reload that rewrites the very slots it
reads.  An upload ordered behind the composite (svr_composite marks itself like a render) leaves it showing the old
state; an unordered one would land first and show through."""
import numpy as np
import pytest
import torch

from composite_twin import composite_twin, material_of, matrices_of
from oracle import lmip
from slice_twin import HIT
from sub_volume_renderer_amd import TransferFunction, testing

pytestmark = pytest.mark.gpu
SLEEP_CYCLES = 300_000_000          # a few tenths of a second of spinning on the GPU clock: far longer than the reload
TF = TransferFunction.from_points([(0.0, (0.2, 0.4, 1.0, 0.0)), (0.5, (1.0, 0.5, 0.2, 0.4)), (1.0, (1.0, 1.0, 1.0, 0.9))])


def _rings_with_roi(orac, roi_from):
    return [dict(r, offset=o["offset"], shape=o["shape"], density=r["density"].copy(), labels=r["labels"].copy())
            for r, o in zip(lmip.rings_of(orac), roi_from)]


def test_a_reload_waits_for_a_composite_still_in_flight():
    spec = testing.synthetic_spec(64, 64, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    vol.material.render_mode, vol.material.transfer_function = "composite", TF
    orac = lmip.oracle_volume(spec)
    old = [dict(r, density=r["density"].copy(), labels=r["labels"].copy()) for r in lmip.rings_of(orac)]
    new_position = (31.5 + 24.0, 31.5 + 20.0, 31.5 + 2.0)
    table = TF.device_table(vol._volume_dimensions)

    def twin(rings):
        return composite_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material),
                              table, 64, 64, 0.99, pick_id=vol.id)

    moved = lmip.oracle_volume(spec)
    moved.center_on_position(new_position)
    expect_old = twin(old)
    torn = twin(_rings_with_roi(moved, old))
    assert (expect_old["flags"] == HIT).sum() > 1000
    assert (np.abs(torn["rgba"] - expect_old["rgba"]) > 1e-3).any(-1).sum() > 100, "the reload must rewrite slots it reads"

    vol.render(cam, 64, 64, count_steps=True)         # the table and the material are on the device before the hold
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)                 # holds the stream: the composite behind it starts much later
        res = vol.render(cam, 64, 64, count_steps=True)
    vol.center_on_position(new_position)                # blocking reload: its uploads are enqueued during the sleep
    s.synchronize()
    got = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "flags", "steps")}
    np.testing.assert_array_equal(got["flags"], expect_old["flags"])
    np.testing.assert_array_equal(got["steps"].view(np.uint32), expect_old["steps"])
    assert np.abs(got["rgba"] - expect_old["rgba"]).max() <= 1e-4

    spec.centers.append((new_position, None))
    orac = lmip.oracle_volume(spec)
    res = vol.render(cam, 64, 64, count_steps=True)
    torch.cuda.synchronize()
    expect_new = twin(lmip.rings_of(orac))
    np.testing.assert_array_equal(res.flags.cpu().numpy(), expect_new["flags"])
    np.testing.assert_array_equal(res.steps.cpu().numpy().view(np.uint32), expect_new["steps"])
    assert np.abs(res.rgba.cpu().numpy() - expect_new["rgba"]).max() <= 1e-4
    vol.close()
