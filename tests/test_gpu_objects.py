"""GPU: svr_objects (include/svr.h) == the numpy restatement of tests/objects_twin.py.  Records are compacted and sorted by
label; every integer field, vmin and vmax are ``array_equal`` to the twin, unused records are all-zero bytes and the
header is equal; on float32 rings value_sum (f64 additions in any order) is held to 2 * finite * 2^-53 * sum|v|.
u8 / u16 / float32 rings whose labels are a hash with ~1900 distinct ids (ids above 2^31, 0 and 0xFFFFFFFF among them),
tables at load 0.47, 0.94 and 1.0, overflowing tables, boxes across the wrap seams, ``selected`` lists, a volume without
label rings, every voxel its own label, a constant ring, a moving window, the micro-block copy, the Python surface,
untouched renders, and every refusal with nothing enqueued."""
import ctypes as C

import numpy as np
import pytest
import torch

from objects_twin import RECORD, box_twin, considered_voxels, objects_twin, position_twin
from oracle import lmip
from sub_volume_renderer_amd import _native as N, _wobject as W, testing

pytestmark = pytest.mark.gpu
f32 = np.float32
WINDOW0 = 48 * 40 * 40
# what the hashed labels give, counted on the CPU through rings_of: (distinct labels, ids above 2^31) per LOD
SCENE_FACTS = {0: (1931, 952), 1: (884, 444)}


def hashed_labels(shape, k):
    """The label volume of the k-th pair: boxes of 5 x 3 x 2 voxels with hashed ids, 30 % label 0, 1 % label 0xFFFFFFFF."""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.uint64) for n in shape), indexing="ij")
    h = ((x // 5) * 73856093 ^ (y // 3) * 19349663 ^ (z // 2) * 83492791 ^ np.uint64(k)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)
    label = h.copy()
    label[h % 10 < 3] = 0
    label[h % 97 == 5] = 0xFFFFFFFF
    return label.astype(np.uint32)


def spec_of(kind):
    spec = testing.synthetic_spec(64, 96, 80)
    if kind == "own":                                                     # every voxel its own label: linear index + 1
        d0 = spec.pairs[0][0]
        own = (np.arange(d0.size, dtype=np.uint32) + np.uint32(1)).reshape(d0.shape)
        spec.pairs = [(d, own if k == 0 else hashed_labels(d.shape, k)) for k, (d, _) in enumerate(spec.pairs)]
        return spec
    spec.pairs = [(d, hashed_labels(d.shape, k)) for k, (d, _) in enumerate(spec.pairs)]
    if kind == "u16":
        spec.pairs = [(d.astype(np.uint16) * np.uint16(251), l) for d, l in spec.pairs]
    if kind == "f32":
        pairs = []
        for k, (d, l) in enumerate(spec.pairs):
            d = d.astype(f32) * f32(0.37) - f32(20.0)                     # negative values too
            flat = d.reshape(-1)
            # the special values go into unlabelled voxels only, so that every labelled object stays finite
            free = np.flatnonzero(np.asarray(l).reshape(-1) == 0)
            if free.size < 650:
                pairs.append((d, l))
                continue
            pick = np.random.default_rng(10 + k).choice(free, 650, replace=False)
            flat[pick[:200]], flat[pick[200:400]], flat[pick[400:600]] = np.nan, np.inf, -np.inf
            flat[pick[600:]] = f32(3e38)
            pairs.append((d, l))
        spec.pairs = pairs
    if kind == "nolabels":
        spec.pairs = [(d, None) for d, _ in spec.pairs]
    if kind == "twin_all":
        spec.blocked_twin = "all"
    if kind == "twin_off":
        spec.blocked_twin = False
    return spec


_SCENES = {}


def scene_of(kind):
    """(volume, rings of the CPU restatement) of a scene, built once per module run."""
    if kind not in _SCENES:
        spec = spec_of(kind)
        vol = testing.build(spec).volume
        assert vol._rings.density_storage == {"u16": "uint16", "f32": "float32"}.get(kind, "uint8")
        _SCENES[kind] = (vol, lmip.rings_of(lmip.oracle_volume(spec)))
    return _SCENES[kind]


_TWINS = {}


def twin_of(kind, lod, box=None, labels=None, ignore_zero=False):
    """The restatement's answer, computed once per distinct question and left unchanged."""
    key = (kind, lod, box, None if labels is None else tuple(labels), ignore_zero)
    if key not in _TWINS:
        _TWINS[key] = objects_twin(scene_of(kind)[1][lod], box, labels, ignore_zero, integer=kind != "f32")
    return _TWINS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for vol, _ in _SCENES.values():
        vol.close()
    _SCENES.clear()
    _TWINS.clear()


def c_objects(vol, lod, capacity, box=None, labels=None, ignore_zero=False):
    """One svr_objects call through the C ABI into sentinel-filled buffers -> (records as RECORD array, header u64 [8])."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    records = torch.full((capacity, 12), -7, dtype=torch.int64, device=dev)
    header = torch.full((8,), -7, dtype=torch.int64, device=dev)
    op = N.ObjectsParams(lod=lod, capacity=capacity, ignore_zero=int(ignore_zero))
    if box is not None:
        op.use_box = 1
        op.box_off[:], op.box_shape[:] = box
    sel = None
    if labels is not None:
        sel = torch.from_numpy(np.unique(np.asarray(labels, np.uint32)).view(np.int32)).to(dev)
        op.selected, op.selected_count = sel.data_ptr(), sel.numel()
    oo = N.ObjectsOutputs(records.data_ptr(), header.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().svr_objects(handle, C.byref(op), C.byref(oo), C.c_void_p(stream)), "svr_objects")
    torch.cuda.synchronize()
    return records.cpu().numpy().view(RECORD).reshape(-1), header.cpu().numpy().view(np.uint64)


def check_records(records, twin, what):
    """The occupied records against the twin's records of their labels; the others all-zero bytes.  -> the occupied ones, by label."""
    used = records[records["used"] != 0]
    assert not records[records["used"] == 0].view(np.uint8).any(), (what, "an unused record is not all-zero")
    assert (used["used"] == 1).all() and not used["reserved"].any(), what
    used = used[np.argsort(used["label"])]
    assert np.unique(used["label"]).size == used.size, (what, "a label owns two records")
    assert all(int(l) in twin["objects"] for l in used["label"]), (what, "a label that is not considered")
    ref = [twin["objects"][int(l)] for l in used["label"]]
    for k in ("voxels", "finite"):
        assert np.array_equal(used[k], np.array([r[k] for r in ref], np.uint64)), (what, k)
    for k, dt in (("sum", np.uint64), ("lo", np.int32), ("hi", np.int32)):
        assert np.array_equal(used[k].reshape(-1, 3), np.array([r[k] for r in ref], dt).reshape(-1, 3)), (what, k)
    for k in ("vmin", "vmax"):
        assert np.array_equal(used[k], np.array([r[k] for r in ref], f32)), (what, k)
    if twin["integer"]:
        assert np.array_equal(used["value_sum"], np.array([r["value_sum"] for r in ref], np.uint64)), (what, "value_sum")
    else:
        got = used["value_sum"].view(np.float64)
        want = np.array([r["value_sum"] for r in ref], np.float64)
        bound = np.array([2.0 * r["finite"] * 2.0 ** -53 * r["abs_sum"] for r in ref], np.float64)
        assert (np.abs(got - want) <= bound).all(), (what, "value_sum", float(np.max(np.abs(got - want) - bound)))
    return used


def same(got, twin, capacity, what):
    """A table that was large enough: every label of the twin has its record, and the header is the twin's."""
    records, header = got
    assert records.size == capacity
    used = check_records(records, twin, what)
    assert used["label"].tolist() == sorted(twin["objects"]), (what, "labels")
    assert [int(v) for v in header.view(np.int64)] == twin["header"], (what, header, twin["header"])
    return used


def test_the_scene_is_what_the_issue_counted():
    for kind in ("u8", "u16", "f32"):
        _, rings = scene_of(kind)
        for lod, (distinct, high) in SCENE_FACTS.items():
            x, y, z, label, value = considered_voxels(rings[lod])
            assert label.size == (WINDOW0 if lod == 0 else 32 ** 3)
            ids, counts = np.unique(label, return_counts=True)
            assert ids.size == distinct and int((ids >= 2 ** 31).sum()) == high
            assert ids[0] == 0 and ids[-1] == 0xFFFFFFFF
            share = counts[0] / label.size
            assert (0.29 < share < 0.31) if lod == 0 else (0.26 < share < 0.28)
            assert counts.min() == (6 if lod == 0 else 8)
            rows = label.reshape(-1, 48 if lod == 0 else 32)
            runs = 1 + (rows[:, 1:] != rows[:, :-1]).sum(axis=1)
            assert abs(rows.shape[1] / runs.mean() - (5.2 if lod == 0 else 4.9)) < 0.06


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("lod", [0, 1])
def test_whole_window(kind, lod):
    vol, _ = scene_of(kind)
    distinct = SCENE_FACTS[lod][0]
    for ignore_zero in (False, True):
        twin = twin_of(kind, lod, ignore_zero=ignore_zero)
        n = distinct - int(ignore_zero)
        assert len(twin["objects"]) == n and (twin["header"][3] > 0) == ignore_zero
        for capacity in (4096, 2048, n):                               # 2048 on LOD 0: load 0.94; n: not one record to spare
            used = same(c_objects(vol, lod, capacity, ignore_zero=ignore_zero), twin, capacity, (kind, lod, capacity, ignore_zero))
            assert int(used["voxels"].sum()) == twin["header"][1]
    if kind == "f32" and lod == 0:
        zero = twin_of(kind, 0)["objects"][0]
        assert zero["finite"] < zero["voxels"] and np.isfinite(zero["vmax"])      # the seeded NaN and infinities sit in label 0


BOXES = [
    ("window", None),
    ("both seams", ((5, 30, 35), (20, 15, 10))),            # y 30..45 and z 35..45 cross ring slot 40 -> 0
    ("odd x", ((3, 10, 12), (29, 7, 5))),
    ("odd x, one slot", ((1, 39, 39), (17, 3, 3))),
    ("partly outside", ((-5, 0, 40), (20, 20, 30))),
    ("outside", ((100, 100, 100), (4, 4, 4))),
    ("beyond int32", ((2**31 - 2, 8, 8), (2**31 - 1, 4, 4))),
    ("one voxel", ((17, 23, 41), (1, 1, 1))),
    ("empty shape", ((4, 10, 10), (0, 5, 5))),
]


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_boxes(kind):
    vol, _ = scene_of(kind)
    for name, box in BOXES:
        twin = twin_of(kind, 0, box=box)
        records, header = c_objects(vol, 0, 2048, box=box)
        same((records, header), twin, 2048, (kind, name))
        if name in ("outside", "beyond int32", "empty shape"):
            assert not records.view(np.uint8).any() and header[:4].tolist() == [0, 0, 0, 0]
        elif name == "one voxel":
            assert header[:2].tolist() == [1, 1]
        else:
            assert header[1] > 100 and header[0] >= 4
    box = ((3, 2, 1), (21, 30, 31))
    same(c_objects(vol, 1, 1024, box=box, ignore_zero=True), twin_of(kind, 1, box=box, ignore_zero=True), 1024, (kind, "lod 1"))


def c_histogram_considered(vol, lod, box=None, labels=None):
    """tail[3] of one svr_histogram call: every voxel it considered, whatever its value."""
    dev = torch.device("cuda", vol._rings.device)
    counts, tail = torch.full((1,), -7, dtype=torch.int64, device=dev), torch.full((4,), -7, dtype=torch.int64, device=dev)
    hp = N.HistogramParams(lod=lod, lo=0.0, hi=256.0, bins=1)
    if box is not None:
        hp.use_box = 1
        hp.box_off[:], hp.box_shape[:] = box
    sel = None
    if labels is not None:
        sel = torch.from_numpy(np.unique(np.asarray(labels, np.uint32)).view(np.int32)).to(dev)
        hp.selected, hp.selected_count = sel.data_ptr(), sel.numel()
    ho = N.HistogramOutputs(counts.data_ptr(), tail.data_ptr(), None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().svr_histogram(vol.prepare(), C.byref(hp), C.byref(ho), C.c_void_p(stream)), "svr_histogram")
    torch.cuda.synchronize()
    return int(tail[3])


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_histogram_and_objects_consider_the_same_voxels(kind):
    """Both passes walk box and window through the same plan (csrc/ring_pieces.h), the histogram in slots of 16 or 4
    voxels aligned to the density ring, the objects pass in slots of 4 aligned to the label ring: the voxels they
    consider are the same, with ignore_zero the dropped label-0 voxels included.  Integers, so ``==``."""
    vol, _ = scene_of(kind)
    ids = sorted(twin_of(kind, 0)["objects"])
    some = [0, ids[len(ids) // 2], 0xFFFFFFFF, ids[len(ids) // 2] + 1]
    for name, box in BOXES:
        for labels in (None, some):
            considered = c_histogram_considered(vol, 0, box, labels)
            _, header = c_objects(vol, 0, 2048, box=box, labels=labels)
            assert considered == int(header[1]), (kind, name, labels)
            _, header = c_objects(vol, 0, 2048, box=box, labels=labels, ignore_zero=True)
            assert considered == int(header[1]) + int(header[3]), (kind, name, labels)
            if labels is None and name == "window":
                assert considered == WINDOW0 and int(header[3]) > 0


def test_selected():
    vol, rings = scene_of("u8")
    ids = sorted(twin_of("u8", 0)["objects"])
    present, absent = ids[len(ids) // 2], ids[len(ids) // 2] + 1
    assert absent not in ids and 0 in ids and 0xFFFFFFFF in ids
    box = ((3, 30, 35), (29, 15, 10))
    for lod in (0, 1):
        for labels in ([present], [0], [0xFFFFFFFF], [absent], [absent, present, 0, 0xFFFFFFFF]):
            for ignore_zero in (False, True):
                twin = twin_of("u8", lod, labels=labels, ignore_zero=ignore_zero)
                same(c_objects(vol, lod, 5, labels=labels, ignore_zero=ignore_zero), twin, 5, ("selected", lod, labels, ignore_zero))
                if labels == [absent]:
                    assert twin["header"][:4] == [0, 0, 0, 0]
                if lod == 0 and 0 in labels:
                    assert (twin["header"][3] > 0) == ignore_zero and (0 in twin["objects"]) != ignore_zero
    inside = [l for l in ids if l and 0 < considered_in(rings[0], box, l) < twin_of("u8", 0)["objects"][l]["voxels"]][:3]
    assert len(inside) == 3                                            # objects the box cuts
    twin = twin_of("u8", 0, box=box, labels=inside + [0], ignore_zero=True)
    same(c_objects(vol, 0, 4, box=box, labels=inside + [0], ignore_zero=True), twin, 4, "selected in a box")
    assert twin["header"][0] == 3 and twin["header"][3] > 0
    # the Python surface sorts and de-duplicates the ids
    table = vol.objects(lod=0, labels=[present, 0xFFFFFFFF, 0, present, absent], background=True)
    assert table.ids.tolist() == [0, present, 0xFFFFFFFF]
    assert table.voxels.tolist() == [twin_of("u8", 0)["objects"][l]["voxels"] for l in (0, present, 0xFFFFFFFF)]


def considered_in(ring, box, label):
    x, y, z, lab, value = considered_voxels(ring, box)
    return int((lab == label).sum())


def test_without_label_rings():
    vol, rings = scene_of("nolabels")
    assert not vol._rings.labels
    off, shape = [int(v) for v in rings[0]["offset"]], [int(v) for v in rings[0]["shape"]]
    used = same(c_objects(vol, 0, 3), twin_of("nolabels", 0), 3, "no labels")
    assert used["label"].tolist() == [0] and used["voxels"].tolist() == [WINDOW0]
    assert used["lo"][0].tolist() == off and used["hi"][0].tolist() == [o + s - 1 for o, s in zip(off, shape)]
    records, header = c_objects(vol, 0, 3, ignore_zero=True)
    same((records, header), twin_of("nolabels", 0, ignore_zero=True), 3, "no labels, ignore_zero")
    assert header[:4].tolist() == [0, 0, 0, WINDOW0] and not records.view(np.uint8).any()
    same(c_objects(vol, 0, 3, labels=[0, 9]), twin_of("nolabels", 0, labels=[0, 9]), 3, "no labels, selected 0")
    assert c_objects(vol, 0, 3, labels=[5])[1][:4].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_overflow(kind):
    vol, _ = scene_of(kind)
    twin = twin_of(kind, 0)
    distinct = SCENE_FACTS[0][0]
    for capacity in (distinct - 1, 7, 1):
        records, header = c_objects(vol, 0, capacity)
        used = check_records(records, twin, (kind, "overflow", capacity))          # complete and exact for its label
        assert used.size == capacity == int(header[0]) and int(header[2]) > 0
        assert int(header[1]) == twin["header"][1] == WINDOW0
        assert int(used["voxels"].sum()) + int(header[2]) == int(header[1])
        assert [int(v) for v in header[3:].view(np.int64)] == twin["header"][3:]


def test_every_voxel_its_own_label():
    vol, _ = scene_of("own")
    twin = twin_of("own", 0)
    assert len(twin["objects"]) == WINDOW0                                          # runs of length 1, more labels than any LDS table
    for capacity in (131072, 81920):
        used = same(c_objects(vol, 0, capacity), twin, capacity, ("own labels", capacity))
        assert (used["voxels"] == 1).all() and np.array_equal(used["lo"], used["hi"])
    records, header = c_objects(vol, 0, 4096)
    used = check_records(records, twin, "own labels, overflow")
    assert int(header[0]) == 4096 and int(header[2]) == WINDOW0 - 4096


def test_moving_window_and_constant_ring():
    """Three moves of the window, which wrap the rings on every axis: every LOD equals the restatement, whole and in a
    box anchored to the moved offset.  Then svr_clear_lod: one record covers the whole window (every lane on one label)."""
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
                same(c_objects(vol, lod, 3000, ignore_zero=ignore_zero), objects_twin(rings[lod], ignore_zero=ignore_zero, integer=True), 3000,
                     (position, lod, ignore_zero))
        box = ((int(rings[0]["offset"][0]) + 3, int(rings[0]["offset"][1]) + 1, int(rings[0]["offset"][2]) + 2), (37, 30, 33))
        same(c_objects(vol, 0, 2048, box=box), objects_twin(rings[0], box=box, integer=True), 2048, (position, "box"))
    off, shape = [int(v) for v in rings[0]["offset"]], [int(v) for v in rings[0]["shape"]]
    window = int(np.prod(shape))
    assert wrapped_x and window > 10000
    lib, handle = N.lib(), vol.prepare()
    N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
    N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
    records, header = c_objects(vol, 0, 16)
    used = records[records["used"] == 1]
    assert header.view(np.int64).tolist() == [1, window, 0, 0, *off, 0] and used.size == 1
    assert not records[records["used"] == 0].view(np.uint8).any()
    r = used[0]
    assert (int(r["label"]), int(r["voxels"]), int(r["finite"]), int(r["value_sum"]), float(r["vmin"]), float(r["vmax"])) == (0, window, window, 0, 0.0, 0.0)
    assert r["lo"].tolist() == off and r["hi"].tolist() == [o + s - 1 for o, s in zip(off, shape)]
    assert r["sum"].tolist() == [window * (s - 1) // 2 for s in shape]
    records, header = c_objects(vol, 0, 16, ignore_zero=True)
    assert header.view(np.int64).tolist() == [0, 0, 0, window, *off, 0] and not records.view(np.uint8).any()
    vol.close()


def test_micro_block_copy_does_not_change_the_table():
    (with_copy, _), (without, _) = scene_of("twin_all"), scene_of("twin_off")
    assert any(with_copy._rings.blocked_twin) and not any(without._rings.blocked_twin)
    for lod in (0, 1):
        a, b = c_objects(with_copy, lod, 2048), c_objects(without, lod, 2048)
        twin = twin_of("twin_all", lod)
        ua, ub = same(a, twin, 2048, ("copy", lod)), same(b, twin, 2048, ("no copy", lod))
        assert ua.tobytes() == ub.tobytes() and a[1].tobytes() == b[1].tobytes()


def test_renders_are_untouched():
    vol, _ = scene_of("u8")
    args = ((31.0, 30.0, 33.0), (0.5, 0.0, 0.0), (0.0, 0.4, 0.3), 96, 80)
    before = {k: getattr(vol.render_slice(*args), k).clone() for k in ("rgba", "value", "label", "flags", "lod")}
    vol.objects(lod=0)
    vol.objects(lod=1, background=True, labels=[0, 5])
    after = vol.render_slice(*args)
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(t.view(torch.uint8), getattr(after, k).view(torch.uint8)), k
    assert int((after.flags == 2).sum()) > 100


def table_equals(table, twin, ring, what):
    ids = sorted(twin["objects"])
    ref = [twin["objects"][l] for l in ids]
    off = [int(v) for v in ring["offset"]]
    assert table.ids.dtype == torch.int64 and table.ids.is_cuda and table.ids.tolist() == ids, what
    assert table.voxels.tolist() == [r["voxels"] for r in ref] and table.finite.tolist() == [r["finite"] for r in ref], what
    assert table.begin.tolist() == [list(r["lo"][::-1]) for r in ref], what
    assert table.end.tolist() == [[v + 1 for v in r["hi"][::-1]] for r in ref], what
    centroid = np.array([[off[a] + r["sum"][a] / r["voxels"] for a in (2, 1, 0)] for r in ref], np.float64).reshape(-1, 3)
    assert table.centroid.dtype == torch.float64 and np.array_equal(table.centroid.cpu().numpy(), centroid), what
    assert np.array_equal(table.min.cpu().numpy(), np.array([r["vmin"] for r in ref], f32)), what
    assert np.array_equal(table.max.cpu().numpy(), np.array([r["vmax"] for r in ref], f32)), what
    mean = table.mean.cpu().numpy()
    if twin["integer"]:
        assert np.array_equal(mean, np.array([r["value_sum"] / r["finite"] for r in ref], np.float64)), what
    else:
        want = np.array([r["value_sum"] / r["finite"] if r["finite"] else np.nan for r in ref], np.float64)
        # the sum's bound divided by finite, and half an ulp for each of the two divisions
        bound = np.array([2.0 * 2.0 ** -53 * r["abs_sum"] for r in ref], np.float64) + 2.0 ** -52 * np.abs(np.nan_to_num(want))
        assert np.array_equal(np.isnan(mean), np.isnan(want)) and (np.abs(mean - want)[~np.isnan(want)] <= bound[~np.isnan(want)]).all(), what
    assert (table.considered, table.background) == (twin["header"][1], twin["header"][3]), what


def test_python_surface(monkeypatch):
    vol, rings = scene_of("u8")
    for lod in (0, 1):
        table = vol.objects(lod=lod)                                               # no background, 4096 records
        twin = twin_of("u8", lod, ignore_zero=True)
        table_equals(table, twin, rings[lod], ("u8", lod))
        assert table.lod == lod and len(table) == SCENE_FACTS[lod][0] - 1 and table.background > 0
        scale = vol.wrapping_buffers[lod].scale_factor
        world = np.asarray(vol.world.matrix, np.float64).tolist()
        ids = sorted(twin["objects"])
        for label in (ids[0], ids[len(ids) // 3], ids[-2], 0xFFFFFFFF):
            rec = twin["objects"][label]
            assert table.box(label) == box_twin(rec["lo"], rec["hi"], scale)
            # the box is ready for histogram(box=): with the id list it counts exactly the object
            assert vol.histogram(lod=lod, box=table.box(label), labels=[label]).considered == rec["voxels"]
            assert table.position(label) == position_twin(rec, rings[lod]["offset"], scale, world)
        with pytest.raises(KeyError):
            table.index(0)                                                         # left out: background=False
        with pytest.raises(KeyError):
            table.index(ids[5] + 1 if ids[5] + 1 not in ids else 1)
    volf, ringsf = scene_of("f32")
    table_equals(volf.objects(lod=0, background=True), twin_of("f32", 0), ringsf[0], "f32")
    box = ((8, 2, 6), (60, 58, 64))                                                # finest scale, numpy order, onto LOD 1
    b, e = W.lod_box(*box, volf.wrapping_buffers[1].scale_factor)
    twin_box = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))
    table_equals(volf.objects(lod=1, box=box), twin_of("f32", 1, box=twin_box, ignore_zero=True), ringsf[1], "f32 box")
    # the automatic capacity: 16 -> 128 -> 1024 -> 8192 records
    calls = []
    lib = N.lib()

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def svr_objects(self, handle, op, oo, stream):
            calls.append(int(op._obj.capacity))
            return lib.svr_objects(handle, op, oo, stream)

    monkeypatch.setattr(W, "_OBJECTS_FIRST_CAPACITY", 16)
    monkeypatch.setattr(N, "lib", lambda: Spy())
    table_equals(vol.objects(lod=0, background=True), twin_of("u8", 0), rings[0], "retry")
    assert calls == [16, 128, 1024, 8192]
    calls.clear()
    assert len(vol.objects(lod=0, labels=[5, 0xFFFFFFFF, 7])) == 1 and calls == [3]       # ids given: one pass, never an overflow
    with pytest.raises(ValueError, match="capacity 100 is too small"):
        vol.objects(lod=0, capacity=100)
    calls.clear()
    table_equals(vol.objects(lod=0, capacity=1931, background=True), twin_of("u8", 0), rings[0], "explicit")
    assert calls == [1931]
    # a caller's side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    table = vol.objects(lod=1, labels=[0xFFFFFFFF, 0], background=True, stream=side.cuda_stream)
    side.synchronize()
    table_equals(table, twin_of("u8", 1, labels=[0, 0xFFFFFFFF]), rings[1], "side stream")


def test_refusals_enqueue_nothing():
    vol, _ = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    records = torch.full((64, 12), -7, dtype=torch.int64, device=dev)
    header = torch.full((8,), -7, dtype=torch.int64, device=dev)
    sel = torch.tensor([0, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        op = N.ObjectsParams(lod=0, capacity=64)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(op, k)[:] = v
            else:
                setattr(op, k, v)
        return op

    def call(op=None, h=handle, null=()):
        op = op or params()
        oo = N.ObjectsOutputs(None if "records" in null else records.data_ptr(), None if "header" in null else header.data_ptr())
        return lib.svr_objects(h, None if "params" in null else C.byref(op), None if "out" in null else C.byref(oo), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("records",)), "null argument"), (dict(null=("header",)), "null argument"),
        (dict(op=params(lod=-1)), "lod out of range"), (dict(op=params(lod=3)), "lod out of range"),
        (dict(op=params(capacity=0)), "capacity must be in"), (dict(op=params(capacity=(1 << 26) + 1)), "capacity must be in"),
        (dict(op=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(op=params(selected=None, selected_count=2)), "NULL selected"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((records == -7).all()) and bool((header == -7).all())              # nothing was enqueued
    # the control cases run: an id list, and a negative box_shape that use_box == 0 makes irrelevant
    assert call(params(selected=sel.data_ptr(), selected_count=2, capacity=2)) == 0
    torch.cuda.synchronize()
    assert header[:4].tolist() == [1, twin_of("u8", 0)["objects"][0]["voxels"], 0, 0] and bool((records[2:] == -7).all())
    assert call(params(box_shape=(4, -1, 4))) == 0
    torch.cuda.synchronize()
    assert int(header[0]) == 64 and int(header[1]) == WINDOW0 and int(header[2]) > 0
