"""GPU: svr_contacts (include/svr.h) == the numpy restatement of tests/contacts_twin.py.  Records are compacted and sorted by
(label_lo, label_hi); every integer field, vmin and vmax are ``array_equal`` to the twin, unused records are all-zero
bytes and all 8 header words are equal; on float32 rings value_sum (f64 additions in any order) is held to
2 * finite * 2^-53 * sum|v|.  The hashed-label scene of test_gpu_objects.py on u8 / u16 / float32 rings at loads of about
0.5, 0.95 and exactly 1.0, overflowing tables, boxes across the wrap seams, boxes of one and two voxels, ``selected``
lists, ``background`` both ways, no label rings, a constant ring, every voxel its own label, the odd rings of
tests/odd_ring_scenes.py, a ring whose rows are longer than one step of a workgroup, a moving window, the micro-block
copy, the Python surface, untouched renders, and every refusal with nothing enqueued."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import odd_ring_scenes as S
import test_gpu_objects as TO
import test_gpu_odd_rings as TR
from contacts_twin import RECORD, box_twin, centroid_twin, contacts_twin, position_twin
from oracle import lmip
from sub_volume_renderer_amd import _native as N, _wobject as W, testing
from sub_volume_renderer_amd._wrapping_buffer import DeviceRings

pytestmark = pytest.mark.gpu
f32, U32 = np.float32, np.uint32
HIGH = 0xFFFFFFFF
WINDOW0 = TO.WINDOW0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")


def spec_of(kind):
    """test_gpu_objects' scenes; on float32 NaN and both infinities are planted in labelled voxels as well (boxes of
    5 x 3 x 2 are all boundary), so that contacts between two objects see values that are not finite."""
    spec = TO.spec_of(kind)
    if kind == "f32":
        for k, (d, l) in enumerate(spec.pairs):
            flat = d.reshape(-1)
            assert np.shares_memory(flat, d)
            labelled = np.flatnonzero(np.asarray(l).reshape(-1) != 0)
            pick = np.random.default_rng(40 + k).choice(labelled, min(600, labelled.size // 4), replace=False)
            third = pick.size // 3
            flat[pick[:third]], flat[pick[third:2 * third]], flat[pick[2 * third:]] = np.nan, np.inf, -np.inf
    return spec


_SCENES, _TWINS, _LONG = {}, {}, []


def scene_of(kind):
    """(volume, rings of the CPU restatement) of a scene, built once per module run."""
    if kind not in _SCENES:
        spec = spec_of(kind)
        vol = testing.build(spec).volume
        assert vol._rings.density_storage == {"u16": "uint16", "f32": "float32"}.get(kind, "uint8")
        _SCENES[kind] = (vol, lmip.rings_of(lmip.oracle_volume(spec)))
    return _SCENES[kind]


def twin_of(kind, lod, box=None, labels=None, ignore_zero=False):
    """The restatement's answer, computed once per distinct question and left unchanged."""
    key = (kind, lod, box, None if labels is None else tuple(labels), ignore_zero)
    if key not in _TWINS:
        _TWINS[key] = contacts_twin(scene_of(kind)[1][lod], box, labels, ignore_zero, integer=kind != "f32")
    return _TWINS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for vol, _ in _SCENES.values():
        vol.close()
    for ctx in list(TR._CONTEXTS.values()) + _LONG:
        ctx.close()
    _SCENES.clear(), _TWINS.clear(), TR._CONTEXTS.clear(), _LONG.clear()


def c_contacts(vol, lod, capacity, box=None, labels=None, ignore_zero=False):
    """One svr_contacts call through the C ABI into sentinel-filled buffers -> (records as RECORD array, header u64 [8])."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    records = torch.full((capacity, 14), -7, dtype=torch.int64, device=dev)
    header = torch.full((8,), -7, dtype=torch.int64, device=dev)
    cp = N.ContactsParams(lod=lod, capacity=capacity, ignore_zero=int(ignore_zero))
    if box is not None:
        cp.use_box = 1
        cp.box_off[:], cp.box_shape[:] = box
    sel = None
    if labels is not None:
        sel = torch.from_numpy(np.unique(np.asarray(labels, np.uint32)).view(np.int32)).to(dev)
        cp.selected, cp.selected_count = sel.data_ptr(), sel.numel()
    co = N.ContactsOutputs(records.data_ptr(), header.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().svr_contacts(handle, C.byref(cp), C.byref(co), C.c_void_p(stream)), "svr_contacts")
    torch.cuda.synchronize()
    return records.cpu().numpy().view(RECORD).reshape(-1), header.cpu().numpy().view(np.uint64)


def keys_of(rec):
    """One u64 per record that orders like (label_lo, label_hi), the twin's order (not the record's own key)."""
    return (rec["label_lo"].astype(np.uint64) << np.uint64(32)) | rec["label_hi"].astype(np.uint64)


def check_records(records, twin, what):
    """The occupied records against the twin's records of their pairs; the others all-zero bytes.  -> the occupied ones, sorted."""
    raw = records.view(np.uint8).reshape(-1, 112)
    occupied = raw[:, :8].any(axis=1)
    assert not raw[~occupied].any(), (what, "an unused record is not all-zero")
    used = records[occupied]
    used = used[np.lexsort((used["label_hi"], used["label_lo"]))]
    assert (used["label_lo"] < used["label_hi"]).all() and not used["reserved"].any(), what
    keys, want_keys = keys_of(used), keys_of(twin["records"])
    assert np.unique(keys).size == keys.size, (what, "a pair owns two records")
    at = np.searchsorted(want_keys, keys)
    assert (at < want_keys.size).all() and np.array_equal(want_keys[np.minimum(at, want_keys.size - 1)], keys), (what, "a pair that is not considered")
    ref = twin["records"][at]
    for k in ("faces", "sum2", "lo", "hi", "finite", "vmin", "vmax"):
        assert np.array_equal(used[k], ref[k]), (what, k, used[k][:4], ref[k][:4])
    if twin["integer"]:
        assert np.array_equal(used["value_sum"], ref["value_sum"]), (what, "value_sum")
        assert np.array_equal(used["finite"], 2 * used["faces"].sum(axis=1)), (what, "finite")
    else:
        got, want = used["value_sum"].view(np.float64), ref["value_sum"].view(np.float64)
        bound = 2.0 * ref["finite"].astype(np.float64) * 2.0 ** -53 * twin["abs_sum"][at]
        assert (np.abs(got - want) <= bound).all(), (what, "value_sum", float(np.max(np.abs(got - want) - bound)))
    return used


def same(got, twin, capacity, what):
    """A table that was large enough: every pair of the twin has its record, and the header is the twin's."""
    records, header = got
    assert records.size == capacity
    used = check_records(records, twin, what)
    assert np.array_equal(keys_of(used), keys_of(twin["records"])), (what, "pairs")
    assert [int(v) for v in header.view(np.int64)] == twin["header"], (what, header, twin["header"])
    return used


# ---- the hashed-label scene ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("lod", [0, 1])
def test_whole_window(kind, lod):
    vol, _ = scene_of(kind)
    for ignore_zero in (False, True):
        twin = twin_of(kind, lod, ignore_zero=ignore_zero)
        pairs = twin["header"][0]
        assert pairs > 500 and (twin["header"][3] > 0) == ignore_zero and twin["header"][7] == (WINDOW0 if lod == 0 else 32 ** 3)
        for capacity in (2 * pairs, pairs * 20 // 19, pairs):          # loads 0.5, 0.95 and 1.0: not one record to spare
            used = same(c_contacts(vol, lod, capacity, ignore_zero=ignore_zero), twin, capacity, (kind, lod, capacity, ignore_zero))
            assert int(used["faces"].sum()) == twin["header"][1]
    rec = twin_of(kind, lod)["records"]
    assert rec["label_lo"][0] == 0 and rec["label_hi"][-1] == HIGH and (rec["label_lo"] >= 2 ** 31).any()
    if kind == "f32":
        short = rec["finite"] < 2 * rec["faces"].sum(axis=1)
        assert short[rec["label_lo"] == 0].any() and short[rec["label_lo"] != 0].any()        # values that are not finite, between objects too


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_overflow(kind):
    vol, _ = scene_of(kind)
    twin = twin_of(kind, 0)
    pairs = twin["header"][0]
    for capacity in (pairs - 1, 7, 1):
        records, header = c_contacts(vol, 0, capacity)
        used = check_records(records, twin, (kind, "overflow", capacity))           # complete and exact for its pair
        assert used.size == capacity == int(header[0]) and int(header[2]) > 0
        assert int(header[1]) == twin["header"][1]
        assert int(used["faces"].sum()) + int(header[2]) == int(header[1])
        assert [int(v) for v in header[3:].view(np.int64)] == twin["header"][3:]


BOXES = [
    ("window", None),
    ("partly outside", ((-5, 0, 40), (20, 20, 30))),
    ("outside", ((100, 100, 100), (4, 4, 4))),
    ("beyond int32", ((2**31 - 2, 8, 8), (2**31 - 1, 4, 4))),
    ("empty shape", ((4, 10, 10), (0, 5, 5))),
]


def seam_boxes(ring):
    """[(name, box)] across the wrap seam of each axis on which the window has one, and across all of them at once;
    an axis without a seam (the window begins at slot 0) gets an odd stretch of the window's inside instead."""
    off, shape = [int(v) for v in ring["offset"]], [int(v) for v in ring["shape"]]
    extent = np.asarray(ring["density"]).shape[::-1]
    seam = [-(-off[a] // extent[a]) * extent[a] for a in range(3)]
    has = [off[a] < seam[a] < off[a] + shape[a] for a in range(3)]
    across = [(max(off[a], seam[a] - 7), 15) if has[a] else (off[a] + 3, 9) for a in range(3)]
    inside = [(off[a] + 3, min(9, seam[a] - off[a] - 3) if has[a] and seam[a] - off[a] > 4 else 9) for a in range(3)]
    out = []
    for a in range(3):
        if has[a]:
            spans = [across[k] if k == a else inside[k] for k in range(3)]
            out.append(("xyz"[a] + " seam", (tuple(s[0] for s in spans), tuple(s[1] for s in spans))))
    out.append(("every seam", (tuple(s[0] for s in across), tuple(s[1] for s in across))))
    return out, has


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_boxes(kind):
    vol, rings = scene_of(kind)
    off = [int(v) for v in rings[0]["offset"]]
    seams, has = seam_boxes(rings[0])
    assert has[1] and has[2] and len(seams) >= 3                   # x wraps in test_moving_window_and_constant_ring and on the odd rings
    odd = [("odd x", ((off[0] + 3, off[1] + 10, off[2] + 12), (29, 7, 5))), ("one row", ((off[0] + 1, off[1] + 9, off[2] + 9), (45, 1, 1)))]
    for name, box in BOXES + odd + seams:
        twin = twin_of(kind, 0, box=box)
        records, header = c_contacts(vol, 0, 8192, box=box)
        same((records, header), twin, 8192, (kind, name))
        if name in ("outside", "beyond int32", "empty shape"):
            assert not records.view(np.uint8).any() and header[:4].tolist() == [0, 0, 0, 0] and int(header[7]) == 0
        elif name == "one row":
            assert header[1] > 5 and int(header[7]) == 45
        else:
            assert header[1] > 100 and header[0] >= 4
    box = ((3, 2, 1), (21, 30, 31))
    same(c_contacts(vol, 1, 2048, box=box, ignore_zero=True), twin_of(kind, 1, box=box, ignore_zero=True), 2048, (kind, "lod 1"))


def test_boxes_of_one_and_two_voxels():
    """1 x 1 x 1 has no face; 2 x 1 x 1, 1 x 2 x 1 and 1 x 1 x 2 have one or none, at places taken from the labels."""
    from contacts_twin import box_block

    vol, rings = scene_of("u8")
    first, lab, _ = box_block(rings[0])
    for axis, dim in ((0, 2), (1, 1), (2, 0)):
        p = tuple(slice(0, -1) if d == dim else slice(None) for d in range(3))
        q = tuple(slice(1, None) if d == dim else slice(None) for d in range(3))
        differ = lab[p] != lab[q]
        shape = tuple(2 if a == axis else 1 for a in range(3))
        for want in (True, False):
            for z, y, x in np.argwhere(differ == want)[[0, 7, -1]]:
                box = ((first[0] + int(x), first[1] + int(y), first[2] + int(z)), shape)
                twin = twin_of("u8", 0, box=box)
                records, header = c_contacts(vol, 0, 3, box=box)
                same((records, header), twin, 3, ("two voxels", box))
                assert header[:2].tolist() == [int(want), int(want)] and int(header[7]) == 2
                if want:
                    assert records[records["label_hi"] != 0]["faces"][0].tolist() == [int(a == axis) for a in range(3)]
                one = (box[0], (1, 1, 1))
                records, header = c_contacts(vol, 0, 3, box=one)
                same((records, header), twin_of("u8", 0, box=one), 3, ("one voxel", one))
                assert header[:2].tolist() == [0, 0] and int(header[7]) == 1


def test_selected_and_background():
    vol, rings = scene_of("u8")
    rec = twin_of("u8", 0)["records"]
    ids = np.unique(np.r_[rec["label_lo"], rec["label_hi"]]).tolist()
    present, absent = ids[len(ids) // 2], ids[len(ids) // 2] + 1
    assert absent not in ids and 0 in ids and HIGH in ids
    for lod in (0, 1):
        for labels in ([present], [0], [HIGH], [absent], [absent, present, 0, HIGH]):
            for ignore_zero in (False, True):
                twin = twin_of("u8", lod, labels=labels, ignore_zero=ignore_zero)
                same(c_contacts(vol, lod, 4096, labels=labels, ignore_zero=ignore_zero), twin, 4096, ("selected", lod, labels, ignore_zero))
                if labels == [absent]:
                    assert twin["header"][:4] == [0, 0, 0, 0]
                if lod == 0 and 0 in labels:
                    assert (twin["header"][3] > 0) == ignore_zero and bool((twin["records"]["label_lo"] == 0).any()) != ignore_zero
    one = twin_of("u8", 0, labels=[present])
    assert 2 <= one["header"][0] <= 30 and ((one["records"]["label_lo"] == present) | (one["records"]["label_hi"] == present)).all()
    box = ((int(rings[0]["offset"][0]) + 3, int(rings[0]["offset"][1]) + 30, int(rings[0]["offset"][2]) + 35), (29, 15, 10))
    twin = twin_of("u8", 0, box=box, labels=[present, 0, HIGH], ignore_zero=True)
    same(c_contacts(vol, 0, 512, box=box, labels=[present, 0, HIGH], ignore_zero=True), twin, 512, "selected in a box")
    assert twin["header"][3] > 0


def test_without_label_rings():
    vol, rings = scene_of("nolabels")
    assert not vol._rings.labels
    off = [int(v) for v in rings[0]["offset"]]
    for kw in (dict(), dict(ignore_zero=True), dict(labels=[0, 9]), dict(labels=[5])):
        records, header = c_contacts(vol, 0, 3, **kw)
        same((records, header), twin_of("nolabels", 0, **kw), 3, ("no labels", kw))
        assert header.view(np.int64).tolist() == [0, 0, 0, 0, *off, WINDOW0] and not records.view(np.uint8).any()


def test_every_voxel_its_own_label():
    """The spill path: far more pairs than any LDS table holds.  The count is known: every face is a pair of its own."""
    vol, _ = scene_of("own")
    twin = twin_of("own", 0)
    nx, ny, nz = 48, 40, 40
    pairs = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1)
    assert twin["header"][:2] == [pairs, pairs] and nx * ny * nz == WINDOW0
    used = same(c_contacts(vol, 0, pairs + pairs // 8), twin, pairs + pairs // 8, "own labels")
    assert (used["faces"].sum(axis=1) == 1).all() and np.array_equal(used["lo"], used["hi"]) and (used["finite"] == 2).all()
    records, header = c_contacts(vol, 0, 4096)
    check_records(records, twin, "own labels, overflow")
    assert int(header[0]) == 4096 and int(header[2]) == pairs - 4096


def test_moving_window_and_constant_ring():
    """Three moves of the window, which wrap the rings on every axis: every LOD equals the restatement, whole and in a
    box anchored to the moved offset.  Then svr_clear_lod: a constant ring has no face."""
    spec = spec_of("u8")
    vol = testing.build(spec).volume
    wrapped_x = False
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        rings = lmip.rings_of(lmip.oracle_volume(spec))
        wrapped_x |= bool(rings[0]["offset"][0] % 48)
        for lod in range(3):
            for ignore_zero in (False, True):
                same(c_contacts(vol, lod, 16384, ignore_zero=ignore_zero), contacts_twin(rings[lod], ignore_zero=ignore_zero, integer=True), 16384,
                     (position, lod, ignore_zero))
        box = ((int(rings[0]["offset"][0]) + 3, int(rings[0]["offset"][1]) + 1, int(rings[0]["offset"][2]) + 2), (37, 30, 33))
        same(c_contacts(vol, 0, 8192, box=box), contacts_twin(rings[0], box=box, integer=True), 8192, (position, "box"))
    off, shape = [int(v) for v in rings[0]["offset"]], [int(v) for v in rings[0]["shape"]]
    assert wrapped_x and int(np.prod(shape)) > 10000
    lib, handle = N.lib(), vol.prepare()
    N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
    N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
    for ignore_zero in (False, True):
        records, header = c_contacts(vol, 0, 16, ignore_zero=ignore_zero)
        assert header.view(np.int64).tolist() == [0, 0, 0, 0, *off, int(np.prod(shape))] and not records.view(np.uint8).any()
    vol.close()


def test_micro_block_copy_does_not_change_the_table():
    (with_copy, _), (without, _) = scene_of("twin_all"), scene_of("twin_off")
    assert any(with_copy._rings.blocked_twin) and not any(without._rings.blocked_twin)
    for lod in (0, 1):
        a, b = c_contacts(with_copy, lod, 16384), c_contacts(without, lod, 16384)
        twin = twin_of("twin_all", lod)
        ua, ub = same(a, twin, 16384, ("copy", lod)), same(b, twin, 16384, ("no copy", lod))
        assert ua.tobytes() == ub.tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- rings aligned to nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(S.SCENES))
def test_odd_rings(key):
    ctx = TR.context(key)
    integer = ctx.scene.storage != "float32"
    picked = S.selections(ctx.scene.has_labels)
    for li, lod, name, (off, shape, ring, dens, labs) in ctx.windows():
        rd = lod.ring_dict(off, shape)
        for labels, ignore_zero in [(None, False), (None, True)] + [(p, False) for p in picked] + [(picked[0] + [0], True)]:
            twin = contacts_twin(rd, None, labels, ignore_zero, integer=integer)
            used = same(c_contacts(ctx, li, 32, labels=labels, ignore_zero=ignore_zero), twin, 32, (key, li, name, labels, ignore_zero))
            assert int(used["faces"].sum()) == twin["header"][1] and twin["header"][4:8] == [*off, int(np.prod(shape))]
        if labs is None:
            assert twin["header"][1] == 0
        else:
            whole = contacts_twin(rd, integer=integer)
            pairs = set(zip(whole["records"]["label_lo"].tolist(), whole["records"]["label_hi"].tolist()))
            if S.run_of(lod.ring[0])[0] and name != "far":
                assert any(S.RUN_LABEL in p for p in pairs)            # the row across the x seam touches its neighbours
            if name.startswith("full") and min(lod.ring) > 4:
                assert any(3 in p for p in pairs) and any(0xFFFFFFF0 in p for p in pairs)      # the objects across the y and z seams


@pytest.mark.parametrize("key", S.BOX_SCENES)
def test_odd_ring_boxes(key):
    ctx = TR.context(key)
    lod, (off, shape, ring, dens, labs), boxes = TR.part_window_and_boxes(ctx)
    rd = lod.ring_dict(off, shape)
    picked = S.selections(True)[0]
    faces = 0
    for name, box in boxes:
        for labels, ignore_zero in ((None, False), (picked, True)):
            twin = contacts_twin(rd, box, labels, ignore_zero, integer=ctx.scene.storage != "float32")
            same(c_contacts(ctx, 0, 32, box=box, labels=labels, ignore_zero=ignore_zero), twin, 32, (key, name, labels, ignore_zero))
            faces += twin["header"][1]
        if name.startswith("row 1 "):
            assert (contacts_twin(rd, box)["records"]["faces"][:, 0] == 0).all()        # rows of one voxel have no x face
    assert faces > 1000


def kernel_constant(file, name):
    text = open(os.path.join(CSRC, file)).read()
    return int(re.search(r"constexpr \w+ " + name + r" = (\d+)u?;", text).group(1))


class LongRows(TR.Context):
    """One raw context whose ring is filled whole from a seeded array: rows of 1099 voxels."""

    RING = (1099, 5, 4)

    def __init__(self):
        rng = np.random.default_rng(77)
        rx, ry, rz = self.RING
        lod = S.Lod.__new__(S.Lod)
        lod.geometry, lod.ring = "long", self.RING
        lod.density = rng.integers(0, 256, (rz, ry, rx)).astype(np.uint8)
        lod.labels = np.array([0, 5, 6, 0xFFFFFFF5], U32)[rng.integers(0, 4, (rz, ry, rx))]
        lod.labels[1, 2, 300:900] = 8                                   # and a run that covers whole waves
        scene = type("Scene", (), {})()
        scene.lods, scene.storage, scene.has_labels, scene.key = [lod], "uint8", True, "long"
        self.scene = scene
        self._rings = DeviceRings([lod.density.shape], density_storage="uint8", labels=True)
        lib, handle = N.lib(), self._rings.handle
        d, lab = np.ascontiguousarray(lod.density), lod.labels
        N.check(lib.svr_upload_region(handle, 0, N.i3((0, 0, 0)), N.i3(lod.ring), C.c_void_p(d.ctypes.data), N.dtype_code(d.dtype),
                                      N.l3(d.strides[::-1]), C.c_void_p(lab.ctypes.data), N.dtype_code(lab.dtype), N.l3(lab.strides[::-1])),
                "svr_upload_region")
        N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")


def test_rows_longer_than_one_step_of_a_workgroup():
    """A workgroup's loop covers kConThreads units of kConUnit voxels per step, and at least kConMinSteps steps: rows of
    1099 voxels put x faces between lanes, between waves, between the steps of one workgroup and, with 20 rows, between
    two workgroups, in the middle of a row."""
    threads, unit, steps = kernel_constant("contacts_kernels.hip", "kConThreads"), kernel_constant("contacts_faces.h", "kConUnit"), \
        kernel_constant("contacts_kernels.hip", "kConMinSteps")
    rx, ry, rz = LongRows.RING
    step = threads * unit
    assert (threads, unit) == (256, 4) and rx > step and rx % unit
    upr = -(-rx // unit)                                                # units of a row (the same at every head here)
    assert upr * ry * rz > threads * steps and 0 < (threads * steps) % upr < upr - 1           # the second workgroup begins inside a row
    ctx = LongRows()
    _LONG.append(ctx)
    lod = ctx.scene.lods[0]
    for off, shape in (((rx, ry, rz), (rx, ry, rz)), ((2 * rx + 1, ry + 1, rz + 2), (rx, ry, rz)), ((3 * rx + 603, 2 * ry + 3, rz + 3), (rx - 2, ry, rz - 1))):
        ctx.set_window(0, off, shape)
        rd = lod.ring_dict(off, shape)
        for ignore_zero in (False, True):
            twin = contacts_twin(rd, ignore_zero=ignore_zero, integer=True)
            used = same(c_contacts(ctx, 0, 16, ignore_zero=ignore_zero), twin, 16, ("long rows", off, ignore_zero))
        rec = {(int(r["label_lo"]), int(r["label_hi"])): r for r in used}
        assert len(rec) == 6 and int(used["faces"][:, 0].sum()) > 0.3 * int(np.prod(shape))     # without label 0: {5, 6, 0xFFFFFFF5, 8}
        lab = lod.window(off, shape)[4]
        for x in (unit - 1, 64 * unit - 1, step - 1, step + unit - 1):            # a lane's, a wave's and a step's last voxel
            assert (lab[:, :, x] != lab[:, :, x + 1]).any()
    box = ((3 * rx + 603 + 2, 2 * ry + 3, rz + 3), (1050, 2, 2))
    same(c_contacts(ctx, 0, 16, box=box, labels=[5, 8]), contacts_twin(rd, box, [5, 8], integer=True), 16, "long rows, box")


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
def test_renders_are_untouched():
    vol, _ = scene_of("u8")
    args = ((31.0, 30.0, 33.0), (0.5, 0.0, 0.0), (0.0, 0.4, 0.3), 96, 80)
    before = {k: getattr(vol.render_slice(*args), k).clone() for k in ("rgba", "value", "label", "flags", "lod")}
    vol.contacts(lod=0)
    vol.contacts(lod=1, background=True, labels=[0, 5])
    after = vol.render_slice(*args)
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(t.view(torch.uint8), getattr(after, k).view(torch.uint8)), k
    assert int((after.flags == 2).sum()) > 100


def table_equals(table, twin, ring, what):
    rec = twin["records"]
    off = [int(v) for v in ring["offset"]]
    assert table.a.dtype == torch.int64 and table.a.is_cuda, what
    assert table.a.tolist() == rec["label_lo"].tolist() and table.b.tolist() == rec["label_hi"].tolist(), what
    assert table.faces.tolist() == rec["faces"][:, ::-1].tolist() and table.area.tolist() == rec["faces"].sum(axis=1).tolist(), what
    assert table.begin.tolist() == rec["lo"][:, ::-1].tolist() and table.end.tolist() == (rec["hi"][:, ::-1] + 1).tolist(), what
    assert table.finite.tolist() == rec["finite"].tolist(), what
    centroid = np.array([centroid_twin(r, off)[::-1] for r in rec], np.float64).reshape(-1, 3)
    assert table.centroid.dtype == torch.float64 and np.array_equal(table.centroid.cpu().numpy(), centroid), what
    assert np.array_equal(table.min.cpu().numpy(), rec["vmin"]) and np.array_equal(table.max.cpu().numpy(), rec["vmax"]), what
    mean = table.mean.cpu().numpy()
    fin = rec["finite"].astype(np.float64)
    if twin["integer"]:
        assert np.array_equal(mean, rec["value_sum"].astype(np.float64) / fin), what
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.where(fin > 0, rec["value_sum"].view(np.float64) / fin, np.nan)
        # the sum's bound divided by finite, and half an ulp for each of the two divisions
        bound = 2.0 * 2.0 ** -53 * twin["abs_sum"] + 2.0 ** -52 * np.abs(np.nan_to_num(want))
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(mean), np.isnan(want)) and (np.abs(mean - want)[ok] <= bound[ok]).all(), what
    assert (table.considered, table.background, table.voxels) == (twin["header"][1], twin["header"][3], twin["header"][7]), what


def test_python_surface(monkeypatch):
    vol, rings = scene_of("u8")
    for lod in (0, 1):
        table = vol.contacts(lod=lod, capacity=16384)                              # no background
        twin = twin_of("u8", lod, ignore_zero=True)
        table_equals(table, twin, rings[lod], ("u8", lod))
        assert table.lod == lod and len(table) == twin["header"][0] and table.background > 0
        scale = vol.wrapping_buffers[lod].scale_factor
        assert table.scale_factor == tuple(float(v) for v in scale)
        world = np.asarray(vol.world.matrix, np.float64).tolist()
        rec = twin["records"]
        for r in (rec[0], rec[len(rec) // 3], rec[-1]):
            a, b = int(r["label_lo"]), int(r["label_hi"])
            assert table.box(b, a) == box_twin(r, scale)
            assert table.position(a, b) == position_twin(r, rings[lod]["offset"], scale, world)
        with pytest.raises(KeyError):
            table.index(0, int(rec[0]["label_hi"]))                                # left out: background=False
    # the surface of an object: its contacts with everything, label 0 included
    whole = vol.contacts(lod=0, background=True, capacity=16384)
    rec = twin_of("u8", 0)["records"]
    some = int(rec["label_hi"][len(rec) // 2])
    mine = (rec["label_lo"] == some) | (rec["label_hi"] == some)
    assert whole.surface(some) == int(rec["faces"][mine].sum()) > 0
    ids, areas = whole.neighbours(some)
    assert sorted(ids.tolist()) == sorted(np.where(rec["label_lo"] == some, rec["label_hi"], rec["label_lo"])[mine].tolist())
    assert areas.tolist() == sorted(areas.tolist(), reverse=True)
    picked = vol.contacts(lod=0, labels=[some, some], background=True)
    table_equals(picked, twin_of("u8", 0, labels=[some]), rings[0], "labels")
    assert picked.surface(some) == whole.surface(some)
    volf, ringsf = scene_of("f32")
    table_equals(volf.contacts(lod=0, background=True, capacity=16384), twin_of("f32", 0), ringsf[0], "f32")
    box = ((8, 2, 6), (60, 58, 64))                                                # finest scale, numpy order, onto LOD 1
    b, e = W.lod_box(*box, volf.wrapping_buffers[1].scale_factor)
    twin_box = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))
    table_equals(volf.contacts(lod=1, box=box), twin_of("f32", 1, box=twin_box, ignore_zero=True), ringsf[1], "f32 box")
    # the automatic capacity: 16 -> 128 -> 1024 -> 8192 records, until every pair of the window has one
    calls = []
    lib = N.lib()

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def svr_contacts(self, handle, cp, co, stream):
            calls.append(int(cp._obj.capacity))
            return lib.svr_contacts(handle, cp, co, stream)

    monkeypatch.setattr(W, "_OBJECTS_FIRST_CAPACITY", 16)
    monkeypatch.setattr(N, "lib", lambda: Spy())
    pairs = twin_of("u8", 0)["header"][0]
    assert 1024 < pairs <= 8192
    table_equals(vol.contacts(lod=0, background=True), twin_of("u8", 0), rings[0], "retry")
    assert calls == [16, 128, 1024, 8192]
    calls.clear()
    table_equals(vol.contacts(lod=0, labels=[some], background=True), twin_of("u8", 0, labels=[some]), rings[0], "labels, retry")
    assert calls[0] == 16                                                          # an id list does not bound the pairs
    with pytest.raises(ValueError, match="capacity 100 is too small"):
        vol.contacts(lod=0, capacity=100)
    calls.clear()
    table_equals(vol.contacts(lod=0, capacity=pairs, background=True), twin_of("u8", 0), rings[0], "explicit")
    assert calls == [pairs]
    # a caller's side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    table = vol.contacts(lod=1, labels=[HIGH, 0], background=True, capacity=4096, stream=side.cuda_stream)
    side.synchronize()
    table_equals(table, twin_of("u8", 1, labels=[0, HIGH]), rings[1], "side stream")


def test_refusals_enqueue_nothing():
    vol, _ = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    records = torch.full((64, 14), -7, dtype=torch.int64, device=dev)
    header = torch.full((8,), -7, dtype=torch.int64, device=dev)
    sel = torch.tensor([0, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        cp = N.ContactsParams(lod=0, capacity=64)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(cp, k)[:] = v
            else:
                setattr(cp, k, v)
        return cp

    def call(cp=None, h=handle, null=()):
        cp = cp or params()
        co = N.ContactsOutputs(None if "records" in null else records.data_ptr(), None if "header" in null else header.data_ptr())
        return lib.svr_contacts(h, None if "params" in null else C.byref(cp), None if "out" in null else C.byref(co), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("records",)), "null argument"), (dict(null=("header",)), "null argument"),
        (dict(cp=params(lod=-1)), "lod out of range"), (dict(cp=params(lod=3)), "lod out of range"),
        (dict(cp=params(capacity=0)), "capacity must be in"), (dict(cp=params(capacity=(1 << 26) + 1)), "capacity must be in"),
        (dict(cp=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(cp=params(selected=None, selected_count=2)), "NULL selected"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode() and "svr_contacts" in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((records == -7).all()) and bool((header == -7).all())              # nothing was enqueued
    # the control cases run: an id list, and a negative box_shape that use_box == 0 makes irrelevant
    twin = twin_of("u8", 0, labels=[0, 5])
    assert call(params(selected=sel.data_ptr(), selected_count=2, capacity=2)) == 0
    torch.cuda.synchronize()
    assert header[:2].tolist() == [2, twin["header"][1]] and int(header[2]) > 0 and bool((records[2:] == -7).all())
    assert call(params(box_shape=(4, -1, 4))) == 0
    torch.cuda.synchronize()
    assert int(header[0]) == 64 and int(header[1]) == twin_of("u8", 0)["header"][1] and int(header[2]) > 0
