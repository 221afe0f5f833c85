"""GPU: the slice, slab, composite and iso kernels of EVERY LOD count 1 .. 8 (SVR_MAX_LODS) == their numpy twins, on the
scenes of tests/lod_scenes.py, in which every LOD 0 .. nl - 1 is the one that resolves samples somewhere
(tests/test_lod_counts.py asserts that on the twins).  The kernels are instantiated per LOD count; the other GPU tests
launch the ones for 1, 2 and 3 LODs only.  What the LOD count parameterises is exercised here: the dispatch
(``with_lods_esh``), the unrolled cascade, the "no LOD" marker of the slab and composite kernels, the per-lane LOD
select under linear sampling, the ``lod`` plane, scales down to 2^-7, and in the iso kernel the chain of the
empty-space test across LODs with and without a cell grid.

Comparisons and tolerances are the mode tests': value, label, flags, lod, steps and pick bit for bit, rgba, depth and
normal within 1e-4, linear value planes bit for bit; iso frames with skipping == without it on every plane, bit for
bit, and the counters show skipped stretches."""
import numpy as np
import pytest
import torch

import lod_scenes as S
from linear_twin import slab_of_spec, slice_of_spec
from oracle import lmip
from slab_twin import MODES, twin_of_spec as slab_twin_of_spec
from slice_twin import HIT, twin_of_spec as slice_twin_of_spec
from sub_volume_renderer_amd import testing
from test_gpu_composite import MID, check as check_composite, composite_on, host as host_render, twin as composite_twin_of
from test_gpu_iso import assert_same_planes, both_ways, check as check_iso, iso_on, twin as iso_twin_of
from test_gpu_linear import check_planes, check_render, check_slice as check_slice_linear, composite_ref, iso_ref
from test_gpu_slab import check as check_slab
from test_gpu_slice import check as check_slice, host as host_slice

pytestmark = pytest.mark.gpu
NLS = list(range(1, S.MAX_LODS + 1))
RING_TYPE = {"u8": "uint8", "u16": "uint16", "f32": "float32"}
CUTOFF = 0.95


def build(nl, storage, kind="pow2", mixed=False):
    spec = S.scene(nl, storage, kind, mixed)
    vol = testing.build(spec).volume
    assert vol._rings.density_storage == RING_TYPE[storage] and len(vol.wrapping_buffers) == nl
    return spec, vol, lmip.oracle_volume(spec)


def is_pow2_volume(vol):
    """svr_launch_slab's predicate for the two-op coordinate chain: every volume extent a power of two."""
    return all(np.frexp(np.float32(s))[0] == 0.5 for s in vol._volume_dimensions)


# ---- slices -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolation", ["nearest", "linear"])
@pytest.mark.parametrize("storage", S.STORAGES)
@pytest.mark.parametrize("nl", NLS)
def test_slices(nl, storage, interpolation):
    spec, vol, orac = build(nl, storage, "odd" if nl % 2 else "pow2")
    for name, origin, u, v in S.slice_planes(spec):
        what = ("slice", nl, storage, interpolation, name)
        res = vol.render_slice(origin, u, v, spec.width, spec.height, interpolation=interpolation)
        torch.cuda.synchronize()
        got = host_slice(res)
        if interpolation == "linear":
            check_slice_linear(got, slice_of_spec(spec, origin, u, v, spec.width, spec.height, vol=orac), what)
        else:
            check_slice(got, slice_twin_of_spec(spec, origin, u, v, spec.width, spec.height, vol=orac), what)
        # a kernel dispatched with fewer LODs than the volume has cannot produce the last slot
        assert int(got["lod"][got["lod"] != 255].max()) == nl - 1, what
    vol.close()


# ---- slabs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(S.KINDS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", NLS)
def test_slabs(nl, mode, kind):
    """Over max / min / mean every (nl, storage) pair appears, each with nearest and linear sampling, on a volume whose
    extents are powers of two (nearest slabs take the two-op coordinate chain) and on one whose are not."""
    storage = S.STORAGES[(nl + MODES.index(mode)) % 3]
    spec, vol, orac = build(nl, storage, kind)
    assert is_pow2_volume(vol) == (kind == "pow2")
    w, samples = S.slab_steps()
    for name, origin, u, v in S.slice_planes(spec):
        what = ("slab", nl, storage, mode, kind, name)
        res = vol.render_slab(origin, u, v, w, samples, spec.width, spec.height, mode=mode)
        torch.cuda.synchronize()
        got = host_slice(res)
        check_slab(got, slab_twin_of_spec(spec, origin, u, v, w, samples, mode, spec.width, spec.height, vol=orac), what)
        assert int(got["lod"][got["lod"] != 255].max()) == nl - 1, what
        res = vol.render_slab(origin, u, v, w, samples, spec.width, spec.height, mode=mode, interpolation="linear")
        torch.cuda.synchronize()
        ref = slab_of_spec(spec, origin, u, v, w, samples, mode, spec.width, spec.height, vol=orac)
        check_planes(host_slice(res), ref, what + ("linear",), ("flags", "label", "lod", "value"), ("rgba", "depth"))
    vol.close()


# ---- composite --------------------------------------------------------------------------------------------------
def composite_frames(vol, spec, orac, what, linear):
    """Both cameras, tint off and on, a cutoff below 1, with the pick and steps planes; ``linear``: also the "top"
    camera under linear sampling."""
    hits = 0
    for cam_name in S.CAMERAS:
        cam = S.camera(spec, cam_name).camera()
        for tint in (False, True):
            vol.material.interpolation = "nearest"
            composite_on(vol, MID, CUTOFF, tint)
            res = vol.render(cam, spec.width, spec.height, count_steps=True, pick=True)
            torch.cuda.synchronize()
            ref = composite_twin_of(vol, cam, spec, orac, MID, CUTOFF, tint)
            check_composite(res, ref, what + (cam_name, tint))
            hits += int((ref["flags"] == HIT).sum())
        if linear and cam_name == "top":
            vol.material.interpolation = "linear"
            got = host_render(vol.render(cam, spec.width, spec.height, count_steps=True, pick=True))
            torch.cuda.synchronize()
            check_render(got, composite_ref(vol, cam, spec, orac, MID, CUTOFF, True), what + (cam_name, "linear"))
            vol.material.interpolation = "nearest"
    return hits


COMPOSITE_CASES = [(nl, S.STORAGES[nl % 3]) for nl in NLS] + [(8, s) for s in S.STORAGES if s != S.STORAGES[8 % 3]]


@pytest.mark.parametrize("nl,storage", COMPOSITE_CASES)
def test_composite(nl, storage):
    spec, vol, orac = build(nl, storage, "pow2" if nl % 2 else "odd")
    assert composite_frames(vol, spec, orac, ("composite", nl, storage), linear=True) > 4 * 32
    vol.close()


# ---- iso --------------------------------------------------------------------------------------------------------
def iso_frames(vol, spec, orac, what, linear):
    """Both cameras at the levels of lod_scenes.ISO_LEVELS: skipping on == off on every plane bit for bit, stretches
    really are skipped, and the frame == the twin; ``linear``: the same under linear sampling at the first level."""
    top = S.vmax("u16" if vol._rings.density_storage == "uint16" else "u8")
    skipped = 0
    for cam_name in S.CAMERAS:
        cam = S.camera(spec, cam_name).camera()
        for interpolation, levels in (("nearest", S.ISO_LEVELS), ("linear", S.ISO_LEVELS[:1] if linear else ())):
            for level in levels:
                iso_on(vol, level * top, iso_refine=4, color_by_label=True)
                vol.material.interpolation = interpolation
                (on, n_on), (off, n_off) = both_ways(vol, cam, spec.width, spec.height)
                w = what + (cam_name, interpolation, level)
                print(w, "wave-stretches marched / skipped with skipping", n_on, "without", n_off)
                assert_same_planes(on, off, w)
                assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0], w
                assert n_on[1] > 0, w
                skipped += int(n_on[1])
                if interpolation == "linear":
                    check_render(on, iso_ref(vol, cam, spec, orac), w)
                else:
                    check_iso(on, iso_twin_of(vol, cam, spec, orac), w)
    vol.material.interpolation = "nearest"
    return skipped


ISO_CASES = ([(nl, S.STORAGES[(nl + 1) % 3], False) for nl in NLS]
             + [(8, s, False) for s in S.STORAGES if s != S.STORAGES[(8 + 1) % 3]]
             + [(4, "u8", True), (8, "u8", True), (8, "f32", True)])


@pytest.mark.parametrize("nl,storage,mixed", ISO_CASES)
def test_iso(nl, storage, mixed):
    """``mixed``: the odd levels have no macro-cell grid (their rings' y extent is no multiple of 8)."""
    spec, vol, orac = build(nl, storage, "pow2" if mixed or nl % 2 == 0 else "odd", mixed)
    rings_zyx = [tuple(int(n) for n in b.texture.shape) for b in orac.wrapping_buffers]
    grids = [not any(r % 8 for r in ring) for ring in rings_zyx]
    assert grids[0] and (all(grids) != (mixed and nl > 1))
    iso_frames(vol, spec, orac, ("iso", nl, storage, mixed), linear=True)
    vol.close()


# ---- window movement --------------------------------------------------------------------------------------------
def test_fly_through_with_eight_lods():
    """Two center_on_position moves after which windows wrap their rings on every axis: composite and iso == the twins."""
    spec, vol, orac = build(S.MAX_LODS, "u8")
    sizes = spec.centers[0][1]
    for k, position in enumerate(S.FLY):
        vol.center_on_position(position, sizes)
        spec.centers.append((position, sizes))
        orac = lmip.oracle_volume(spec)
        last = k == len(S.FLY) - 1
        composite_frames(vol, spec, orac, ("fly composite", position), linear=last)
        iso_frames(vol, spec, orac, ("fly iso", position), linear=last)
    w = S.wraps(orac)
    assert all(w[0]) and all(any(lod[a] for lod in w[1:]) for a in range(3)), w
    vol.close()
