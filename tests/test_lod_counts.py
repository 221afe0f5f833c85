"""CPU: the scenes of tests/lod_scenes.py reach every LOD slot.  tests/test_gpu_lod_counts.py launches the slice, slab,
composite and iso kernels of every LOD count 1 .. 8 on these scenes; a kernel instantiated for NL LODs is only
exercised where each of its NL cascade arms is the one that resolves a sample.  That is a property of the scenes, so it
is asserted here, on the numpy twins, for every LOD count, both volume shapes and the mixed grid / no-grid variant:

- slices: over the planes the GPU test uses, the ``lod`` plane shows every LOD 0 .. nl - 1 on at least 32 pixels, and
  some pixels inside the volume that no LOD holds (255);
- composite and iso: every LOD resolves samples (the twins' per-LOD census), under both cameras;
- iso: over the levels and cameras the GPU test uses, hits lie in the finest LOD, a middle one and the coarsest;
- windows: some window wraps its ring on every axis, the fly-through's last window does on every axis, and the mixed
  variant has gridded and grid-less levels with LOD 0 gridded.

The twins do not model empty-space skipping (a skipped stretch must not change a plane), so nothing is asserted about
it here."""
import numpy as np
import pytest

import composite_twin
import iso_twin
import lod_scenes as S
import slab_twin
import slice_twin
from oracle import lmip
from sub_volume_renderer_amd import TransferFunction

HIT = slice_twin.HIT
MIN_PIXELS = 32
NLS = list(range(1, S.MAX_LODS + 1))
TF = TransferFunction.from_points([(0.0, (0.1, 0.2, 0.9, 0.0)), (0.3, (0.2, 0.9, 0.3, 0.08)), (0.6, (1.0, 0.6, 0.1, 0.3)),
                                   (1.0, (1.0, 1.0, 1.0, 0.6))], size=64)


def gridded(ring_zyx):
    """Does svr_create give a LOD with this ring a macro-cell grid (every extent a multiple of 8)?"""
    return not any(r % 8 for r in ring_zyx)


@pytest.mark.parametrize("kind", list(S.KINDS))
@pytest.mark.parametrize("mixed", [False, True], ids=["gridded", "mixed"])
def test_geometry(kind, mixed):
    levels, focus = S.geometry(kind, mixed)
    base = S.KINDS[kind]
    assert levels[0]["shape"] == base and levels[-1]["shape"][2] * 128 == base[2]         # x scale down to 2^-7
    grids = [gridded([r * c for r, c in zip(L["ring"], L["chunk"])]) for L in levels]
    assert grids[0]
    assert grids == ([l % 2 == 0 for l in range(S.MAX_LODS)] if mixed else [True] * S.MAX_LODS)
    # the windows the builder predicts are the ones the ring restatement loads, and they are nested shells: in data
    # voxels each window contains the finer one along x and reaches beyond it (on y and z the coarse levels are a few
    # voxels thick and their windows are what the chunk grid leaves of the requested share)
    spec = S.scene(S.MAX_LODS, "u8", kind, mixed)
    orac = lmip.oracle_volume(spec)
    wins = S.windows(kind, mixed)
    for b, (o, s) in zip(orac.wrapping_buffers, wins):
        assert b.current_logical_roi_in_pixels == (o, s)
    spans = []
    for L, (o, s) in zip(levels, wins):
        vox = [bb // ss for bb, ss in zip(base, L["shape"])]
        spans.append([(oo * v, (oo + ss) * v) for oo, ss, v in zip(o, s, vox)])
    for fine, coarse in zip(spans, spans[1:]):
        assert coarse[2][0] <= fine[2][0] and fine[2][1] <= coarse[2][1]
        assert coarse[2][0] < fine[2][0] or fine[2][1] < coarse[2][1]
    assert spans[-1][2][0] > 0 and spans[-1][2][1] < base[2]                               # room no LOD holds
    w = S.wraps(orac)
    assert all(any(lod[a] for lod in w) for a in range(3)), w
    assert all(w[0]), w                                                                    # the finest: on every axis


@pytest.mark.parametrize("kind", list(S.KINDS))
@pytest.mark.parametrize("nl", NLS)
def test_slices_and_slabs_show_every_lod(nl, kind):
    spec = S.scene(nl, "u8", kind)
    orac = lmip.oracle_volume(spec)
    for name, origin, u, v in S.slice_planes(spec):
        ref = slice_twin.twin_of_spec(spec, origin, u, v, spec.width, spec.height, vol=orac)
        counts = np.bincount(ref["lod"].ravel(), minlength=256)
        # each plane on its own shows every shell
        assert (counts[:nl] >= MIN_PIXELS).all() and counts[255] >= MIN_PIXELS, (name, counts[:nl], counts[255])
        assert counts[nl:255].sum() == 0
        assert (ref["flags"] == slice_twin.MISS).sum() >= MIN_PIXELS                       # inside the volume, no LOD
    w, samples = S.slab_steps()
    name, origin, u, v = S.slice_planes(spec)[1]
    for mode in slab_twin.MODES:
        ref = slab_twin.twin_of_spec(spec, origin, u, v, w, samples, mode, spec.width, spec.height, vol=orac)
        counts = np.bincount(ref["lod"].ravel(), minlength=256)
        assert (counts[:nl] > 0).all() and counts[255] > 0, (mode, counts[:nl])


def ray_twins(spec, orac, levels):
    """The composite twin and the iso twin at ``levels`` (fractions of the value range) for the spec's camera."""
    rings = lmip.rings_of(orac)
    size = orac.volume_dimensions_shader
    table = TF.device_table(np.array(size, np.float32))
    comp = composite_twin.composite_twin(rings, spec.matrices(), size, composite_twin.material_of(spec.material), table,
                                         spec.width, spec.height, 0.95, True, census=True)
    top = spec.material["clim"][1]
    isos = [iso_twin.iso_twin(rings, spec.matrices(), size, iso_twin.material_of(spec.material), spec.width, spec.height,
                              dict(iso_value=f * top), census=True) for f in levels]
    return comp, isos


ISO_LEVELS = S.ISO_LEVELS


@pytest.mark.parametrize("kind,mixed", [("pow2", False), ("odd", False), ("pow2", True)])
@pytest.mark.parametrize("nl", NLS)
def test_rays_resolve_and_hit_at_every_lod(nl, kind, mixed):
    spec = S.scene(nl, "u8", kind, mixed)
    orac = lmip.oracle_volume(spec)
    hit_lods = set()
    for cam in S.CAMERAS:
        S.camera(spec, cam)
        comp, isos = ray_twins(spec, orac, ISO_LEVELS)
        assert (comp["census"] > 0).all(), (cam, comp["census"])
        print(nl, kind, mixed, cam, "composite hit pixels", int((comp["flags"] == HIT).sum()), "census", comp["census"])
        assert (comp["flags"] == HIT).sum() >= MIN_PIXELS and (comp["flags"] != HIT).sum() >= MIN_PIXELS
        for ref in isos:
            assert (ref["census"] > 0).all(), (cam, ref["census"])
            print(nl, kind, mixed, cam, "iso hit pixels", int((ref["flags"] == HIT).sum()), "census", ref["census"])
            assert (ref["flags"] == HIT).any()
            hit_lods |= set(np.unique(ref["hit_lod"][ref["hit_lod"] >= 0]).tolist())
        # (one LOD's window is a small part of the frame: the count is over the levels)
        assert sum(int((ref["flags"] == HIT).sum()) for ref in isos) >= MIN_PIXELS
    assert {0, nl // 2, nl - 1} <= hit_lods, hit_lods


def test_the_fly_through_wraps_every_axis():
    spec = S.scene(S.MAX_LODS)
    sizes = spec.centers[0][1]
    for position in S.FLY:
        spec.centers.append((position, sizes))
    orac = lmip.oracle_volume(spec)
    w = S.wraps(orac)
    assert all(w[0]) and all(any(lod[a] for lod in w[1:]) for a in range(3)), w
    for cam in S.CAMERAS:
        S.camera(spec, cam)
        comp, isos = ray_twins(spec, orac, ISO_LEVELS[:1])
        assert (comp["census"] > 0).all() and (isos[0]["census"] > 0).all()


def test_the_census_changes_nothing():
    spec = S.scene(3)
    orac = lmip.oracle_volume(spec)
    rings, size = lmip.rings_of(orac), orac.volume_dimensions_shader
    table = TF.device_table(np.array(size, np.float32))
    args = (rings, spec.matrices(), size, composite_twin.material_of(spec.material))
    a = composite_twin.composite_twin(*args, table, spec.width, spec.height, 0.95, True)
    b = composite_twin.composite_twin(*args, table, spec.width, spec.height, 0.95, True, census=True)
    assert set(b) - set(a) == {"census"} and int(b["census"].sum()) > 0
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    a = iso_twin.iso_twin(*args, spec.width, spec.height, dict(iso_value=80.0))
    b = iso_twin.iso_twin(*args, spec.width, spec.height, dict(iso_value=80.0), census=True)
    assert set(b) - set(a) == {"census", "hit_lod"}
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert ((b["hit_lod"] >= 0) == (b["flags"] == HIT)).all()
