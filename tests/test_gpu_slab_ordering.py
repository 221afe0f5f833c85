"""GPU: a slab still in flight is never overwritten under it.  The slab's stream is held by a bounded sleep kernel, so
the slab runs only well after the host has enqueued a blocking ring reload that rewrites the very slots it reads.  An
upload ordered behind the slab (svr_slab marks itself like a render) leaves it showing the old state; an unordered one
would land first and show through.  Also: slab output tensors are kept per frame size."""
import numpy as np
import pytest
import torch

from oracle import lmip
from slab_twin import twin_of_spec
from slice_twin import HIT
from sub_volume_renderer_amd import SubVolume, testing

pytestmark = pytest.mark.gpu
SLEEP_CYCLES = 300_000_000          # a few tenths of a second of spinning on the GPU clock: far longer than the reload


def _rings_with_roi(orac, roi_from):
    return [dict(r, offset=o["offset"], shape=o["shape"], density=r["density"].copy(), labels=r["labels"].copy())
            for r, o in zip(lmip.rings_of(orac), roi_from)]


def test_a_reload_waits_for_a_slab_still_in_flight():
    spec = testing.synthetic_spec(64, 64, 64)
    vol = testing.build(spec).volume
    orac = lmip.oracle_volume(spec)
    old = [dict(r, density=r["density"].copy(), labels=r["labels"].copy()) for r in lmip.rings_of(orac)]
    slab = SubVolume.axis_slab_plane("z", (31.5, 31.5, 33.0), 1.0, 1.0)
    n, mode = 7, "max"
    new_position = (31.5 + 24.0, 31.5 + 20.0, 33.0 + 2.0)

    moved = lmip.oracle_volume(spec)
    moved.center_on_position(new_position)
    expect_old = twin_of_spec(spec, *slab, n, mode, 64, 64, vol=orac, rings=old)
    torn = twin_of_spec(spec, *slab, n, mode, 64, 64, vol=moved, rings=_rings_with_roi(moved, old))
    assert (expect_old["flags"] == HIT).sum() > 1000
    assert (torn["value"] != expect_old["value"]).sum() > 100, "the reload must rewrite slots this slab reads"

    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)                 # holds the stream: the slab behind it starts much later
        res = vol.render_slab(*slab, n, 64, 64, mode=mode)
    vol.center_on_position(new_position)                # blocking reload: its uploads are enqueued during the sleep
    s.synchronize()
    for k in ("value", "lod", "flags", "depth"):
        np.testing.assert_array_equal(getattr(res, k).cpu().numpy(), expect_old[k], err_msg=k)

    spec.centers.append((new_position, None))
    orac = lmip.oracle_volume(spec)
    res = vol.render_slab(*slab, n, 64, 64, mode=mode)
    torch.cuda.synchronize()
    expect_new = twin_of_spec(spec, *slab, n, mode, 64, 64, vol=orac)
    for k in ("value", "lod", "flags", "depth"):
        np.testing.assert_array_equal(getattr(res, k).cpu().numpy(), expect_new[k], err_msg=k)


def test_slab_output_tensors_are_kept_per_frame_size_apart_from_the_slices():
    spec = testing.synthetic_spec(64, 64, 64)
    vol = testing.build(spec).volume
    orac = lmip.oracle_volume(spec)
    focus = spec.centers[0][0]
    views = [("z", 64, 48), ("y", 64, 40), ("x", 48, 40)]
    first = {}
    slice_ptrs = set()
    for _ in range(3):
        for axis, w, h in views:
            slab = SubVolume.axis_slab_plane(axis, focus, 1.0, 1.0)
            slice_ptrs.add(vol.render_slice(*slab[:3], w, h).rgba.data_ptr())
            res = vol.render_slab(*slab, 5, w, h, mode="mean")
            ptrs = tuple(getattr(res, k).data_ptr() for k in ("rgba", "depth", "label", "flags", "value", "lod"))
            assert first.setdefault((w, h), ptrs) == ptrs, (axis, w, h)
            torch.cuda.synchronize()
            ref = twin_of_spec(spec, *slab, 5, "mean", w, h, vol=orac)
            np.testing.assert_array_equal(res.value.cpu().numpy(), ref["value"])
    assert len(first) == 3 and len(slice_ptrs) == 3
    assert not slice_ptrs & {p[0] for p in first.values()}
