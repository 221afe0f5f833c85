"""GPU: an iso render still in flight is never overwritten under it.  Its stream is held by a bounded sleep kernel, so
the render runs only well after the host has enqueued a blocking ring reload that rewrites the very slots (and the
cell maxima) it reads.  An upload ordered behind the render (svr_iso marks itself like a render) leaves it showing the
old state; an unordered one would land first and show through."""
import numpy as np
import pytest
import torch

from iso_twin import iso_twin, material_of, matrices_of, params_of
from oracle import lmip
from slice_twin import HIT
from sub_volume_renderer_amd import testing

pytestmark = pytest.mark.gpu
SLEEP_CYCLES = 300_000_000          # a few tenths of a second of spinning on the GPU clock: far longer than the reload


def _rings_with_roi(orac, roi_from):
    return [dict(r, offset=o["offset"], shape=o["shape"], density=r["density"].copy(), labels=r["labels"].copy())
            for r, o in zip(lmip.rings_of(orac), roi_from)]


def test_a_reload_waits_for_an_iso_render_still_in_flight():
    spec = testing.synthetic_spec(64, 64, 64)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    m.render_mode, m.iso_value, m.color_by_label = "iso", 0.45 * float(spec.material.get("clim", (0.0, 1.0))[1]), True
    orac = lmip.oracle_volume(spec)
    old = [dict(r, density=r["density"].copy(), labels=r["labels"].copy()) for r in lmip.rings_of(orac)]
    new_position = (31.5 + 24.0, 31.5 + 20.0, 31.5 + 2.0)

    def twin(rings):
        return iso_twin(rings, matrices_of(vol, cam), orac.volume_dimensions_shader, material_of(spec.material), 64, 64,
                        params_of(m), pick_id=vol.id)

    moved = lmip.oracle_volume(spec)
    moved.center_on_position(new_position)
    expect_old = twin(old)
    torn = twin(_rings_with_roi(moved, old))
    assert (expect_old["flags"] == HIT).sum() > 1000
    assert ((np.abs(torn["rgba"] - expect_old["rgba"]) > 1e-3).any(-1).sum() > 100), "the reload must rewrite slots it reads"

    vol.render(cam, 64, 64, count_steps=True)         # the material is on the device before the hold
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)                 # holds the stream: the render behind it starts much later
        res = vol.render(cam, 64, 64, count_steps=True)
    vol.center_on_position(new_position)                # blocking reload: its uploads are enqueued during the sleep
    s.synchronize()
    got = {k: getattr(res, k).cpu().numpy() for k in ("rgba", "flags", "steps", "label")}
    np.testing.assert_array_equal(got["flags"], expect_old["flags"])
    np.testing.assert_array_equal(got["steps"].view(np.uint32), expect_old["steps"])
    np.testing.assert_array_equal(got["label"].view(np.uint32), expect_old["label"])
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
