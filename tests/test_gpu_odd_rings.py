"""GPU: svr_histogram, svr_objects, svr_components, svr_distance and svr_mesh on rings whose extents are aligned to
nothing (tests/odd_ring_scenes.py): x = 63, 21, 42, 36, 40, 3 and 1 voxels, u8 / u16 / float32 storage, with and without
label rings, and 63 and 21 as LOD 0 and LOD 1 of one context.  Rows then start anywhere in a 16-byte slot and in a unit
of 4 ring slots, differently from row to row; a whole unit can sit at an unaligned address; behind the wrap seam the
units lie at no multiple of 4; rows of 3 and of 1 voxel hold no whole unit at all.  Each window (a whole ring's worth at
offsets whose x is 0 .. 3 modulo 4, a part of it that wraps on all three axes, the same part just below 2^31) and each
box is taken through the C ABI and held to the pass's twin with the comparison of that pass's own GPU test, imported
from it: the helpers there ask a volume for ``prepare()`` and ``_rings`` only, which Context provides, so they are
neither restated here nor changed there.  The contexts are raw (DeviceRings, one host upload per ring, windows through
svr_set_lod_state); what the twins are given is cut from the uploaded numpy arrays, not read back.  The read-back is
held to the same arrays on the side."""
import ctypes as C

import numpy as np
import pytest

import odd_ring_scenes as S
import test_gpu_components as TC
import test_gpu_distance as TD
import test_gpu_histogram as TH
import test_gpu_mesh as TM
import test_gpu_objects as TO
from histogram_twin import histogram_twin
from objects_twin import objects_twin
from sub_volume_renderer_amd import _native as N
from sub_volume_renderer_amd._wrapping_buffer import DeviceRings

pytestmark = pytest.mark.gpu
f32, U32 = np.float32, np.uint32
KEYS = list(S.SCENES)


class Context:
    """One raw context with the scene's rings uploaded whole and published.  ``prepare()`` and ``_rings`` are what the
    call helpers of the five GPU test modules ask of a volume."""

    def __init__(self, key):
        self.scene = S.scene(key)
        self._rings = DeviceRings([lod.density.shape for lod in self.scene.lods], density_storage=self.scene.storage, labels=self.scene.has_labels)
        lib, handle = N.lib(), self._rings.handle
        for li, lod in enumerate(self.scene.lods):
            d, lab = np.ascontiguousarray(lod.density), lod.labels
            largs = [None, 0, N.l3((0, 0, 0))] if lab is None else [C.c_void_p(lab.ctypes.data), N.dtype_code(lab.dtype), N.l3(lab.strides[::-1])]
            N.check(lib.svr_upload_region(handle, li, N.i3((0, 0, 0)), N.i3(lod.ring), C.c_void_p(d.ctypes.data), N.dtype_code(d.dtype),
                                          N.l3(d.strides[::-1]), *largs), "svr_upload_region")
        N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")

    def prepare(self):
        return self._rings.handle

    def set_window(self, li, off, shape):
        st = N.LodState()
        st.offset[:], st.shape[:], st.scale[:] = off, shape, (1.0, 1.0, 1.0)
        N.check(N.lib().svr_set_lod_state(self._rings.handle, li, C.byref(st)), "svr_set_lod_state")

    def read(self, li, off, shape):
        """svr_read_region of ring slots [off, off + shape) -> (density f32, labels u32), pattern-filled before."""
        d, lab = np.full(shape[::-1], -5.0, f32), np.full(shape[::-1], 0xABCDEF01, U32)
        N.check(N.lib().svr_read_region(self._rings.handle, li, N.i3(off), N.i3(shape), C.c_void_p(d.ctypes.data), C.c_void_p(lab.ctypes.data)),
                "svr_read_region")
        return d, lab

    def windows(self):
        """Sets each window of each LOD in turn -> (LOD, its scene half, window name, the window as the helpers take it)."""
        for li, lod in enumerate(self.scene.lods):
            for name, off, shape in S.windows(lod.geometry):
                self.set_window(li, off, shape)
                yield li, lod, name, lod.window(off, shape)

    def close(self):
        self._rings.close()


_CONTEXTS = {}


def context(key):
    if key not in _CONTEXTS:
        _CONTEXTS[key] = Context(key)
    return _CONTEXTS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx in _CONTEXTS.values():
        ctx.close()
    _CONTEXTS.clear()


def same_bits(got, want, what):
    assert np.array_equal(got.view(U32), np.asarray(want, f32).view(U32)), (what, int((got.view(U32) != np.asarray(want, f32).view(U32)).sum()))


# ---- upload and read-back at these pitches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_upload_and_read_back(key):
    ctx = context(key)
    for li, lod in enumerate(ctx.scene.lods):
        d, lab = ctx.read(li, (0, 0, 0), lod.ring)
        same_bits(d, lod.density.astype(f32), (key, li, "the whole ring"))
        assert np.array_equal(lab, lod.labels if lod.labels is not None else np.zeros(lab.shape, U32)), (key, li, "labels of the whole ring")
    for li, lod, name, (off, shape, ring, dens, labs) in ctx.windows():
        if name not in ("part", "far"):
            continue
        # the window, piece by piece, put together where the pieces belong
        got_d, got_l = np.full(shape[::-1], -5.0, f32), np.full(shape[::-1], 0xABCDEF01, U32)
        for s, n in S.pieces_of(lod.ring, off, shape):
            at = tuple(slice((s[a] - off[a]) % lod.ring[a], (s[a] - off[a]) % lod.ring[a] + n[a]) for a in (2, 1, 0))
            got_d[at], got_l[at] = ctx.read(li, s, n)
        same_bits(got_d, dens, (key, li, name))
        assert np.array_equal(got_l, labs if labs is not None else np.zeros(got_l.shape, U32)), (key, li, name, "labels")


# ---- every window of every scene -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_histogram(key):
    ctx = context(key)
    for li, lod, name, (off, shape, ring, dens, labs) in ctx.windows():
        rings = {li: lod.ring_dict(off, shape)}
        lo, hi = lod.tails_range()
        for bins in (7, 256):
            for labels in [None] + S.selections(ctx.scene.has_labels):
                ref = histogram_twin(rings, li, lo, hi, bins, labels=labels)
                TH.same(TH.c_hist(ctx, li, lo, hi, bins, labels=labels), ref, (key, li, name, bins, labels))
                read = np.zeros(dens.shape, U32) if labs is None else labs
                assert int(ref["tail"][3]) == (dens.size if labels is None else int(np.isin(read, labels).sum())), (key, li, name, labels)
                if labels is None and dens.size >= 64:
                    assert ref["tail"][0] > 0 and ref["tail"][1] > 0
                    assert ref["counts"][bins - 1] > 0 or not (dens == f32(hi)).any()      # hi is a value of the ring: the closed top bin


@pytest.mark.parametrize("key", KEYS)
def test_objects(key):
    ctx = context(key)
    integer = ctx.scene.storage != "float32"
    picked = S.selections(ctx.scene.has_labels)
    for li, lod, name, (off, shape, ring, dens, labs) in ctx.windows():
        rd = lod.ring_dict(off, shape)
        for labels, ignore_zero in [(None, False), (None, True)] + [(p, False) for p in picked] + [(picked[0] + [0], True)]:
            twin = objects_twin(rd, None, labels, ignore_zero, integer=integer)
            used = TO.same(TO.c_objects(ctx, li, 16, labels=labels, ignore_zero=ignore_zero), twin, 16, (key, li, name, labels, ignore_zero))
            assert int(used["voxels"].sum()) == twin["header"][1] and twin["header"][4:7] == list(off)
        if labs is not None and S.run_of(lod.ring[0])[0] and name != "far":
            assert S.RUN_LABEL in twin["objects"]                      # the row of solid lanes across the x seam is in the window


@pytest.mark.parametrize("key", KEYS)
def test_components(key):
    ctx = context(key)
    level = S.LEVEL[ctx.scene.storage]
    for li, lod, name, window in ctx.windows():
        for connectivity in (6, 26):
            TC.hold(ctx, li, (key, li, name, "level", connectivity), window=window, level=level, connectivity=connectivity)
            TC.hold(ctx, li, (key, li, name, "every label", connectivity), window=window, connectivity=connectivity)
            for picked in S.selections(ctx.scene.has_labels):
                TC.hold(ctx, li, (key, li, name, "selected", connectivity), window=window, selected=picked, ignore_zero=True, connectivity=connectivity)
        TC.hold(ctx, li, (key, li, name, "joined"), window=window, selected=[9, 10, 1, 0], join_labels=True, connectivity=6)


@pytest.mark.parametrize("key", KEYS)
def test_distance(key):
    ctx = context(key)
    level = S.LEVEL[ctx.scene.storage]
    for li, lod, name, window in ctx.windows():
        for mode in (dict(level=level), dict(selected=S.selections(ctx.scene.has_labels)[0])):
            for border in (False, True):
                for invert in (False, True):
                    twin = TD.hold(ctx, li, (key, li, name, tuple(mode), border, invert), window=window, border=border, invert=invert, **mode)
                    assert twin["header"][2] == int(np.prod(window[1])) and twin["header"][4:7] == list(window[0])


@pytest.mark.parametrize("key", KEYS)
def test_mesh(key):
    ctx = context(key)
    for li, lod, name, window in ctx.windows():
        for picked in S.selections(ctx.scene.has_labels):
            TM.hold(ctx, li, (key, li, name, "labels"), window=window, labels=picked)
        twin = TM.hold(ctx, li, (key, li, name, "level"), window=window, level=S.LEVEL[ctx.scene.storage])
        assert twin["header"][4:7] == list(window[0])


# ---- boxes in the W-part window of odd3 ------------------------------------------------------------------------------------
def part_window_and_boxes(ctx):
    lod = ctx.scene.lods[0]
    name, off, shape = S.windows(lod.geometry)[4]
    assert name == "part"
    ctx.set_window(0, off, shape)
    return lod, lod.window(off, shape), S.boxes(off, shape, lod.ring)


@pytest.mark.parametrize("key", S.BOX_SCENES)
def test_boxes_histogram_and_objects(key):
    ctx = context(key)
    lod, (off, shape, ring, dens, labs), boxes = part_window_and_boxes(ctx)
    rd = lod.ring_dict(off, shape)
    lo, hi = lod.tails_range()
    picked = S.selections(True)[0]
    for name, box in boxes:
        for labels in (None, picked):
            ref = histogram_twin({0: rd}, 0, lo, hi, 256, box=box, labels=labels)
            TH.same(TH.c_hist(ctx, 0, lo, hi, 256, box=box, labels=labels), ref, (key, name, labels))
        assert int(ref["tail"][3]) > 0
        for labels, ignore_zero in ((None, False), (picked, True)):
            twin = objects_twin(rd, box, labels, ignore_zero, integer=ctx.scene.storage != "float32")
            TO.same(TO.c_objects(ctx, 0, 16, box=box, labels=labels, ignore_zero=ignore_zero), twin, 16, (key, name, labels, ignore_zero))
        assert twin["header"][1] > 0


@pytest.mark.parametrize("key", S.BOX_SCENES)
def test_boxes_components_distance_and_mesh(key):
    ctx = context(key)
    lod, window, boxes = part_window_and_boxes(ctx)
    level = S.LEVEL[ctx.scene.storage]
    picked = S.selections(True)[0]
    for k, (name, box) in enumerate(boxes):
        TC.hold(ctx, 0, (key, name, "level"), window=window, box=box, level=level, connectivity=26 if k % 2 else 6)
        TC.hold(ctx, 0, (key, name, "labels"), window=window, box=box, selected=[9, 10, 1, 2], connectivity=6 if k % 2 else 26)
        TD.hold(ctx, 0, (key, name, "level"), window=window, box=box, level=level, border=bool(k % 2), invert=bool(k % 3 == 0))
        TD.hold(ctx, 0, (key, name, "labels"), window=window, box=box, selected=picked, border=not k % 2, invert=bool(k % 3 == 1))
        TM.hold(ctx, 0, (key, name, "labels"), window=window, box=box, labels=picked)
        TM.hold(ctx, 0, (key, name, "level"), window=window, box=box, level=level)
