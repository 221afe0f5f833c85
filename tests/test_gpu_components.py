"""GPU: svr_components (include/svr.h) == the numpy restatement tests/components_twin.py, which reads the same window
through svr_read_region: the header, the dense numbers and every field of every record are equal exactly, in every case.
The scene (tests/components_scenes.py): a ring of 72 x 16 x 40 voxels (LOD 1: 36 x 12 x 20) whose window wraps on all
three axes, objects across each seam and across the corner where the seams meet, a one-voxel path that crosses all three
seams, two voxels that touch at a corner across a seam, two labels face to face, a checkerboard; u8, u16 and float32
rings (NaN and infinities planted); a volume without label rings; boxes of 1, 3, 4, 5 and 65 voxels along x at every
alignment; more components than the scan's block size squared; capacities; reproducibility; two streams; ordering behind
uploads; the Python surface; every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from components_scenes import CHECKER, CORNER_PAIR, FACE_PAIR, HIGH, LEVEL, PLANTED, checkerboard_spec, path_voxels, spec_of
from components_twin import RECORD, components_twin
from sub_volume_renderer_amd import Roi, _native as N, testing

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "sub_volume_renderer_amd", "csrc", "components_plan.h")).read()
SCAN_BLOCK = int(re.search(r"kCompScanBlock = (\d+);", PLAN).group(1))
FILL = 0x5A5A5A5A

_SCENES, _WINDOWS = {}, {}


def scene_of(kind):
    if kind not in _SCENES:
        _SCENES[kind] = testing.build(spec_of(kind)).volume
    return _SCENES[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for vol in _SCENES.values():
        vol.close()
    _SCENES.clear()
    _WINDOWS.clear()


def window_of(vol, lod, fresh=False):
    """(offset (x, y, z), shape, ring (numpy order), density f32 [z][y][x], labels u32 or None) of the LOD's window, through
    svr_read_region of the whole ring and the window's ring slots; read once per volume and LOD unless ``fresh``."""
    key = (id(vol), lod)
    if fresh or key not in _WINDOWS:
        st = N.LodState()
        N.check(N.lib().svr_get_lod_state(vol.prepare(), lod, C.byref(st)), "svr_get_lod_state")
        off, shape = [int(v) for v in st.offset], [int(v) for v in st.shape]
        buf = vol.wrapping_buffers[lod]
        ring = tuple(int(v) for v in buf.shape_in_pixels)
        dens, labs = buf.read_ring(Roi((0, 0, 0), ring))
        idx = np.ix_(*[(off[a] + np.arange(shape[a])) % ring[2 - a] for a in (2, 1, 0)])
        _WINDOWS[key] = (off, shape, ring, dens[idx], labs[idx] if vol._rings.labels else None)
    return _WINDOWS[key]


def c_components(vol, lod, *, box=None, level=None, selected=None, ignore_zero=False, join_labels=False, connectivity=6, ids_cap=None,
                 rec_cap=None, stream=None):
    """One svr_components call through the C ABI into pattern-filled arrays of the given capacities (None: NULL and 0)
    -> (header as 16 Python ints, ids u32 [ids_cap] or None, records RECORD [rec_cap] or None)."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    cp = N.ComponentsParams(lod=lod, connectivity=connectivity, ignore_zero=int(ignore_zero), join_labels=int(join_labels))
    if box is not None:
        cp.use_box = 1
        cp.box_off[:], cp.box_shape[:] = box
    sel = None
    if level is not None:
        cp.mode, cp.level = N.COMPONENTS_LEVEL, level
    else:
        cp.mode = N.COMPONENTS_LABELS
        if selected is not None:
            sel = torch.from_numpy(np.unique(np.asarray(selected, np.uint32)).view(np.int32)).to(dev)
            cp.selected, cp.selected_count = sel.data_ptr(), sel.numel()
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    ids = None if ids_cap is None else torch.from_numpy(np.full(ids_cap, FILL, np.uint32).view(np.int32)).to(dev)
    records = None if rec_cap is None else torch.from_numpy(np.full((rec_cap, 20), FILL, np.uint32).view(np.int32)).to(dev)
    co = N.ComponentsOutputs(None if ids is None else ids.data_ptr(), ids_cap or 0, None if records is None else records.data_ptr(), rec_cap or 0,
                             header.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    N.check(N.lib().svr_components(handle, C.byref(cp), C.byref(co), C.c_void_p(s)), "svr_components")
    torch.cuda.synchronize()
    return ([int(v) for v in header.cpu().numpy().view(np.uint64)], None if ids is None else ids.cpu().numpy().view(np.uint32),
            None if records is None else records.cpu().numpy().view(np.uint32).reshape(-1).view(RECORD))


def same_records(got, want, what):
    for name in RECORD.names:
        assert np.array_equal(got[name], want[name]), (what, name)


def hold(vol, lod, what, *, window=None, **mode):
    """Count, then emit into exact capacities, and hold both to the twin.  -> the twin's result."""
    off, shape, ring, dens, labs = window or window_of(vol, lod)
    twin = components_twin(off, dens, labs, **mode)
    want = twin["header"]
    head, _, _ = c_components(vol, lod, **mode)
    assert head == want[:2] + [0, 0] + want[4:], (what, "count", head, want)
    head, ids, records = c_components(vol, lod, ids_cap=max(want[2], 1), rec_cap=max(want[0], 1), **mode)
    assert head == want, (what, head, want)
    assert np.array_equal(ids[:want[2]], twin["ids"].reshape(-1)), (what, "ids", int((ids[:want[2]] != twin["ids"].reshape(-1)).sum()))
    same_records(records[:want[0]], twin["records"], what)
    assert (ids[want[2]:] == FILL).all() and (records[want[0]:].view(np.uint32) == FILL).all(), (what, "beyond the end")
    return twin


def test_the_window_wraps_on_all_three_axes_and_holds_what_was_planted():
    for kind in ("u8", "f32"):
        vol = scene_of(kind)
        for lod in (0, 1):
            off, shape, ring, dens, labs = window_of(vol, lod)
            assert ring == ((40, 16, 72) if lod == 0 else (20, 12, 36))
            for a in range(3):
                assert off[a] % ring[2 - a] + shape[a] > ring[2 - a], (lod, a, off, shape)
    off, shape, ring, dens, labs = window_of(scene_of("u8"), 0)
    path = path_voxels()
    assert int((labs == PLANTED["path"]).sum()) == len(path) and int((labs == PLANTED["corner"]).sum()) == 2
    assert int((labs == 6).sum()) == 1 and int((labs == 7).sum()) == 1 and int((labs == PLANTED["checker"]).sum()) == 16 * 8 * 8 // 2
    for axis, seam in enumerate((72, 32, 40)):                         # the path lies on both sides of every seam
        c = np.array(path)[:, axis]
        assert c.min() < seam <= c.max()
    assert int((labs == 0xFFFFFFF0).sum()) > 30 and int((labs == 1).sum()) > 300
    dens = window_of(scene_of("f32"), 0)[3]
    assert np.isnan(dens).any() and np.isposinf(dens).any() and np.isneginf(dens).any()


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("connectivity", [6, 26])
def test_level_mode(kind, connectivity):
    vol = scene_of(kind)
    for lod in (0, 1):
        off, shape, ring, dens, labs = window_of(vol, lod)
        twin = hold(vol, lod, (kind, lod, "level"), level=LEVEL[kind], connectivity=connectivity)
        assert 0.3 < twin["header"][1] / float(np.prod(shape)) < 0.7 and twin["header"][0] > 1
        assert twin["records"]["voxels"].max() > twin["header"][1] // 4              # one giant component, and specks
        twin = hold(vol, lod, (kind, lod, "high level"), level=HIGH[kind], connectivity=connectivity)
        assert twin["header"][0] > 10
        if lod == 0 and kind == "u8":                                  # the path is one of the components
            assert len(path_voxels()) in twin["records"]["voxels"]
    if kind == "f32":
        for level in (-np.inf, np.inf, 3e38, -25.0):
            hold(vol, 0, (kind, "level", level), level=float(level), connectivity=connectivity)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_label_modes(connectivity):
    vol = scene_of("u8")
    for lod in (0, 1):
        every = hold(vol, lod, (lod, "every label"), connectivity=connectivity)
        assert every["header"][13] == 0 and every["header"][1] == every["header"][2] and 0 in every["records"]["label"]
        no_zero = hold(vol, lod, (lod, "ignore_zero"), ignore_zero=True, connectivity=connectivity)
        assert no_zero["header"][13] > 0 and no_zero["header"][1] + no_zero["header"][13] == every["header"][1]
        picked = hold(vol, lod, (lod, "selected"), selected=[1, 2, 3, 0xFFFFFFF0, 77], connectivity=connectivity)
        assert set(picked["records"]["label"].tolist()) == {1, 2, 3, 0xFFFFFFF0}
        if lod == 0:
            assert picked["header"][0] == 4                            # every seam object is one piece
        with_zero = hold(vol, lod, (lod, "selected with zero dropped"), selected=[0, 9], ignore_zero=True, connectivity=connectivity)
        assert with_zero["header"][13] > 0 and set(with_zero["records"]["label"].tolist()) == {9}
        joined = hold(vol, lod, (lod, "joined"), selected=[9, 10, 1], join_labels=True, connectivity=connectivity)
        split = hold(vol, lod, (lod, "split"), selected=[9, 10, 1], connectivity=connectivity)
        assert joined["header"][0] < split["header"][0] and joined["header"][1] == split["header"][1]
        hold(vol, lod, (lod, "everything joined"), join_labels=True, connectivity=connectivity)


def test_planted_structures_across_the_seams():
    vol = scene_of("u8")
    path = hold(vol, 0, "path, 6", selected=[PLANTED["path"]], connectivity=6)
    assert path["header"][:2] == [1, len(path_voxels())] and path["records"]["first"][0].tolist() == list(min(path_voxels(), key=lambda p: p[::-1]))
    assert hold(vol, 0, "path, 26", selected=[PLANTED["path"]], connectivity=26)["header"][0] == 1
    assert hold(vol, 0, "corner, 6", selected=[PLANTED["corner"]], connectivity=6)["header"][:2] == [2, 2]
    corner = hold(vol, 0, "corner, 26", selected=[PLANTED["corner"]], connectivity=26)
    assert corner["header"][:2] == [1, 2] and corner["records"]["lo"][0].tolist() == list(CORNER_PAIR[0]) and corner["records"]["hi"][0].tolist() == list(CORNER_PAIR[1])
    for connectivity in (6, 26):
        face = hold(vol, 0, "face to face", selected=list(PLANTED["face"]), connectivity=connectivity)
        assert face["header"][:2] == [2, 2] and face["records"]["label"].tolist() == [6, 7]
        face = hold(vol, 0, "face to face, joined", selected=list(PLANTED["face"]), join_labels=True, connectivity=connectivity)
        assert face["header"][:2] == [1, 2] and face["records"]["label"].tolist() == [6] and face["records"]["first"][0].tolist() == list(FACE_PAIR[0])
    # whole-box patterns
    n = CHECKER[1][0] * CHECKER[1][1] * CHECKER[1][2]
    assert hold(vol, 0, "checkerboard, 6", box=CHECKER, selected=[PLANTED["checker"]], connectivity=6)["header"][:2] == [n // 2, n // 2]
    assert hold(vol, 0, "checkerboard, 26", box=CHECKER, selected=[PLANTED["checker"]], connectivity=26)["header"][:2] == [1, n // 2]
    assert hold(vol, 0, "checkerboard, level", box=CHECKER, level=HIGH["u8"], connectivity=6)["header"][0] == n // 2
    for connectivity in (6, 26):
        off, shape = window_of(vol, 0)[:2]
        assert hold(vol, 0, "all inside", join_labels=True, connectivity=connectivity)["header"][:2] == [1, int(np.prod(shape))]
        assert hold(vol, 0, "all inside, level", level=0.0, connectivity=connectivity)["header"][0] == 1
        assert hold(vol, 0, "none inside", selected=[123456], connectivity=connectivity)["header"][:4] == [0, 0, int(np.prod(shape)), 0]
        assert hold(vol, 0, "none inside, level", level=1e9, connectivity=connectivity)["header"][:2] == [0, 0]


def test_box_shapes_and_alignments():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    assert shape[0] >= 69
    seam = ring[2] - off[0] % ring[2]                                  # the window's x at which the ring wraps
    for nx in (1, 3, 4, 5, 65):
        for start in sorted({0, 1, 2, 3, 4, max(seam - 2, 0), max(seam - 1, 0)}):      # every alignment in the ring, and rows that begin just before the seam
            if start + nx > shape[0]:
                continue
            box = ((off[0] + start, off[1] + 3, off[2] + 20), (nx, 9, 25 if nx < 65 else 7))
            mode = dict(level=LEVEL["u8"]) if (nx + start) % 2 else dict(selected=[9, 10, 1])
            hold(vol, 0, ("row", nx, start), box=box, connectivity=26 if start % 2 else 6, **mode)
    hold(vol, 0, "partly outside", box=((off[0] - 5, off[1] + 2, off[2] + shape[2] - 6), (20, shape[1] + 9, 30)), level=LEVEL["u8"])
    hold(vol, 0, "one voxel", box=((off[0] + 7, off[1] + 3, off[2] + 9), (1, 1, 1)), join_labels=True)
    for name, box in (("misses", ((off[0] + shape[0] + 4, off[1], off[2]), (4, 4, 4))), ("empty shape", ((off[0] + 4, off[1] + 2, off[2] + 2), (0, 5, 5)))):
        twin = hold(vol, 0, name, box=box, level=1.0)
        assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7:] == [0] * 9
    # a window of None
    spec = spec_of("u8")
    spec.centers = []
    bare = testing.build(spec).volume
    try:
        head, _, _ = c_components(bare, 0, level=1.0, ids_cap=4, rec_cap=4)
        assert head == [0] * 16
        assert components_twin((0, 0, 0), None, None, level=1.0)["header"] == head
    finally:
        bare.close()


def test_without_label_rings():
    vol = scene_of("nolabels")
    assert not vol._rings.labels
    for lod in (0, 1):
        off, shape, ring, dens, labs = window_of(vol, lod)
        assert labs is None
        solid = hold(vol, lod, "every label reads 0", connectivity=6)
        assert solid["header"][:2] == [1, int(np.prod(shape))] and solid["records"]["label"].tolist() == [0]
        dropped = hold(vol, lod, "and is dropped", ignore_zero=True)
        assert dropped["header"][:2] == [0, 0] and dropped["header"][13] == int(np.prod(shape))
        assert hold(vol, lod, "{5}", selected=[5])["header"][:2] == [0, 0]
        hold(vol, lod, "level", level=LEVEL["u8"], connectivity=26)


def test_every_level_of_the_scan_runs_more_than_one_block():
    vol = testing.build(checkerboard_spec()).volume
    try:
        window = window_of(vol, 0)
        assert window[1] == [128, 64, 64]
        twin = hold(vol, 0, "checkerboard", window=window, selected=[1], connectivity=6)
        assert twin["header"][0] == 128 * 64 * 64 // 2 > SCAN_BLOCK ** 2
        assert -(-twin["header"][2] // SCAN_BLOCK) > SCAN_BLOCK           # level 0 of the scan has block sums in more than one block
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_capacities():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    for mode in (dict(selected=[1, 2, 3, 9]), dict(level=LEVEL["u8"], connectivity=26)):
        twin = components_twin(off, dens, labs, **mode)
        want = twin["header"]
        n_ids, n_rec = want[2], want[0]
        assert n_rec > 10 and n_ids == int(np.prod(shape))
        head, ids, rec = c_components(vol, 0, ids_cap=n_ids - 1, rec_cap=n_rec, **mode)                    # ids one too small: records alone
        assert head == want[:2] + [0, n_rec] + want[4:] and (ids == FILL).all()
        same_records(rec, twin["records"], "records alone")
        head, ids, rec = c_components(vol, 0, ids_cap=n_ids, rec_cap=n_rec - 1, **mode)                    # records one too small: ids alone
        assert head == want[:2] + [n_ids, 0] + want[4:] and (rec.view(np.uint32) == FILL).all()
        assert np.array_equal(ids, twin["ids"].reshape(-1))
        head, ids, rec = c_components(vol, 0, ids_cap=n_ids - 1, rec_cap=n_rec - 1, **mode)
        assert head == want[:2] + [0, 0] + want[4:] and (ids == FILL).all() and (rec.view(np.uint32) == FILL).all()
        head, ids, rec = c_components(vol, 0, ids_cap=n_ids + 3, rec_cap=n_rec + 2, **mode)
        assert head == want and np.array_equal(ids[:n_ids], twin["ids"].reshape(-1)) and (ids[n_ids:] == FILL).all()
        same_records(rec[:n_rec], twin["records"], "larger")
        assert (rec[n_rec:].view(np.uint32) == FILL).all()
        head, ids, rec = c_components(vol, 0, ids_cap=n_ids, **mode)                                     # no records asked for
        assert head == want[:2] + [n_ids, 0] + want[4:] and np.array_equal(ids, twin["ids"].reshape(-1))
        head, ids, rec = c_components(vol, 0, rec_cap=n_rec, **mode)
        assert head == want[:2] + [0, n_rec] + want[4:]
        same_records(rec, twin["records"], "no ids asked for")


def test_two_calls_and_two_streams_give_identical_bytes():
    vol = scene_of("u8")
    dev = torch.device("cuda", vol._rings.device)
    off, shape, ring, dens, labs = window_of(vol, 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for mode in (dict(level=LEVEL["u8"]), dict(ignore_zero=True, connectivity=26)):
        twin = hold(vol, 0, "first", **mode)
        n_ids, n_rec = twin["header"][2], twin["header"][0]
        runs = [c_components(vol, 0, ids_cap=n_ids, rec_cap=n_rec, **mode) for _ in range(2)]
        runs += [c_components(vol, 0, ids_cap=n_ids, rec_cap=n_rec, stream=s.cuda_stream, **mode) for s in streams]
        for head, ids, rec in runs:
            assert head == twin["header"] and ids.tobytes() == twin["ids"].tobytes() and rec.tobytes() == twin["records"].tobytes()
    # two calls in flight on two streams at once: the second is ordered behind the first in the shared scratch
    handle = vol.prepare()
    outs = []
    torch.cuda.synchronize()
    for s, level in zip(streams, (LEVEL["u8"], HIGH["u8"])):
        twin = components_twin(off, dens, labs, level=level)
        cp = N.ComponentsParams(lod=0, connectivity=6, mode=N.COMPONENTS_LEVEL, level=level)
        header = torch.full((16,), -7, dtype=torch.int64, device=dev)
        ids = torch.zeros(twin["header"][2], dtype=torch.int32, device=dev)
        rec = torch.zeros((twin["header"][0], 20), dtype=torch.int32, device=dev)
        outs.append((twin, header, ids, rec))
        torch.cuda.synchronize()
        co = N.ComponentsOutputs(ids.data_ptr(), ids.numel(), rec.data_ptr(), rec.shape[0], header.data_ptr())
        N.check(N.lib().svr_components(handle, C.byref(cp), C.byref(co), C.c_void_p(s.cuda_stream)), "svr_components")
    torch.cuda.synchronize()
    for twin, header, ids, rec in outs:
        assert [int(v) for v in header.cpu().numpy().view(np.uint64)] == twin["header"]
        assert ids.cpu().numpy().view(np.uint32).tobytes() == twin["ids"].tobytes() and rec.cpu().numpy().tobytes() == twin["records"].tobytes()


def test_a_call_right_after_an_upload_sees_it():
    vol = testing.build(spec_of("u8")).volume
    try:
        lib, handle = N.lib(), vol.prepare()
        buf = vol.wrapping_buffers[0]
        rng = np.random.default_rng(2)
        for step in range(2):
            block_d = rng.integers(0, 256, (16, 8, 24)).astype(np.uint8)
            block_l = rng.integers(0, 3, (16, 8, 24)).astype(np.uint32)
            buf._upload(Roi((8 * step, 4, 16 * step), (16, 8, 24)), block_d, block_l)
            N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
            got = [c_components(vol, 0, selected=[1, 2]), c_components(vol, 0, level=100.0, connectivity=26)]
            window = window_of(vol, 0, fresh=True)
            assert got[0][0][:2] == components_twin(window[0], window[3], window[4], selected=[1, 2])["header"][:2], step
            assert got[1][0][:2] == components_twin(window[0], window[3], window[4], level=100.0, connectivity=26)["header"][:2], step
            hold(vol, 0, ("after upload", step), window=window, ignore_zero=True)
        N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
        N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
        shape = window_of(vol, 0)[1]
        assert c_components(vol, 0, level=1.0)[0][:2] == [0, 0]
        assert c_components(vol, 0)[0][:2] == [1, int(np.prod(shape))]
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_python_surface():
    vol = scene_of("u8")
    vol.world.scale = (1.5, 0.5, 2.0)
    vol.world.position = (3.0, -2.0, 7.0)
    try:
        for lod, kw, mode in ((0, dict(level=HIGH["u8"], connectivity=26), dict(level=HIGH["u8"], connectivity=26)),
                              (1, dict(labels=[9, 1, 9]), dict(selected=[1, 9], ignore_zero=True)),
                              (0, dict(background=True, join=True, box=((20, 26, 50), (44, 36, 90))), dict(join_labels=True))):
            off, shape, ring, dens, labs = window_of(vol, lod)
            if "box" in kw:
                b, e = kw["box"]
                mode["box"] = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))               # LOD 0: scale 1
            twin = components_twin(off, dens, labs, **mode)
            got = vol.components(lod=lod, **kw)
            r, head = twin["records"], twin["header"]
            assert got.ids.is_cuda and got.ids.dtype == torch.int32 and tuple(got.ids.shape) == twin["ids"].shape
            assert np.array_equal(got.ids.cpu().numpy(), twin["ids"].astype(np.int32))
            assert (got.count, len(got), got.inside_voxels, got.background, got.lod) == (head[0], head[0], head[1], head[13], lod)
            assert tuple(got.begin) == tuple(head[7:10][::-1]) and tuple(got.offset) == tuple(off[::-1])
            assert np.array_equal(got.label.cpu().numpy(), r["label"]) and np.array_equal(got.voxels.cpu().numpy(), r["voxels"].astype(np.int64))
            for name, want in (("first", r["first"]), ("lo", r["lo"]), ("end", r["hi"] + 1)):
                assert np.array_equal(getattr(got, name).cpu().numpy(), want[:, ::-1]), name
            centroid = (np.array(off, np.float64) + r["sum"] / r["voxels"][:, None].astype(np.float64))
            assert np.array_equal(got.centroid.cpu().numpy(), centroid[:, ::-1])
            order = sorted(range(len(r)), key=lambda k: (-int(r["voxels"][k]), k))
            assert got.largest(5) == [k + 1 for k in order[:5]]
            big = got.largest()[0]
            scale = np.array(vol.wrapping_buffers[lod].scale_factor, np.float64)
            lo, end = r["lo"][big - 1][::-1], r["hi"][big - 1][::-1] + 1
            assert got.box(big) == (tuple(int(v) for v in np.floor(lo / scale)), tuple(int(v) for v in np.ceil(end / scale)))
            data = (centroid[big - 1] + 0.5) / scale[::-1] - 0.5
            assert np.allclose(got.position(big), data * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0]), rtol=0, atol=1e-9)
            assert np.array_equal(got.mask([big]).cpu().numpy(), twin["ids"] == big) and got.mask([big]).is_cuda
            label = int(r["label"][big - 1])
            assert got.pieces(label) == [int(k) + 1 for k in np.nonzero(r["label"] == label)[0]]
            # the first voxel of a component, as a world position, is in it
            for k in (1, big, head[0]):
                c = r["first"][k - 1].astype(np.float64)
                world = ((c + 0.5) / scale[::-1] - 0.5) * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0])
                assert got.id_at(world) == k
            assert got.id_at((-1e5, 0.0, 0.0)) == 0
        path = vol.components(labels=[PLANTED["path"]])
        assert path.count == 1 and int(path.voxels[0]) == len(path_voxels()) and path.pieces(PLANTED["path"]) == [1]
        empty = vol.components(labels=[123456])
        assert empty.count == 0 and len(empty) == 0 and empty.largest(3) == [] and not bool(empty.ids.any()) and tuple(empty.voxels.shape) == (0,)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        again = vol.components(labels=[PLANTED["corner"]], connectivity=26, stream=side.cuda_stream)
        side.synchronize()
        assert again.count == 1 and int(again.voxels[0]) == 2
    finally:
        vol.world.scale = (1.0, 1.0, 1.0)
        vol.world.position = (0.0, 0.0, 0.0)


def test_refusals_enqueue_nothing():
    vol = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((64,), -7, dtype=torch.int32, device=dev)
    records = torch.full((4, 20), -7, dtype=torch.int32, device=dev)
    sel = torch.tensor([1, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        cp = N.ComponentsParams(lod=0, mode=N.COMPONENTS_LABELS, selected=sel.data_ptr(), selected_count=2, connectivity=6)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(cp, k)[:] = v
            else:
                setattr(cp, k, v)
        return cp

    def call(cp=None, h=handle, null=(), ids_cap=64, rec_cap=4):
        cp = cp or params()
        co = N.ComponentsOutputs(None if "ids" in null else ids.data_ptr(), ids_cap, None if "records" in null else records.data_ptr(), rec_cap,
                                 None if "header" in null else header.data_ptr())
        return lib.svr_components(h, None if "params" in null else C.byref(cp), None if "out" in null else C.byref(co), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("header",)), "null argument"),
        (dict(cp=params(lod=-1)), "lod out of range"), (dict(cp=params(lod=2)), "lod out of range"),
        (dict(cp=params(mode=2)), "unknown mode"), (dict(cp=params(mode=-1)), "unknown mode"),
        (dict(cp=params(connectivity=18)), "connectivity must be 6 or 26"), (dict(cp=params(connectivity=0)), "connectivity must be 6 or 26"),
        (dict(cp=params(mode=N.COMPONENTS_LEVEL, level=float("nan"))), "level must not be NaN"),
        (dict(cp=params(selected=None)), "NULL selected pointer"),
        (dict(cp=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(null=("ids",)), "NULL ids"), (dict(null=("records",)), "NULL records"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((ids == -7).all()) and bool((records == -7).all())          # nothing was enqueued
    # more than SVR_COMPONENTS_MAX_VOXELS voxels: the whole window of a u8 ring of 1032 x 1024 x 1024 voxels without labels, on
    # a context of its own, whose memory no kernel touches
    desc = (N.LodDesc * 1)()
    desc[0].ring_dims[:] = (1032, 1024, 1024)
    desc[0].density_storage, desc[0].no_labels, desc[0].blocked_twin = N.SVR_U8, 1, 0
    other = C.c_void_p()
    N.check(lib.svr_create(vol._rings.device, 1, desc, C.byref(other)), "svr_create")
    try:
        st = N.LodState()
        st.offset[:], st.shape[:], st.scale[:] = (0, 0, 0), (1032, 1024, 1024), (1.0, 1.0, 1.0)
        N.check(lib.svr_set_lod_state(other, 0, C.byref(st)), "svr_set_lod_state")
        assert call(cp=params(selected=None, selected_count=0), h=other) == -1
        assert "more than SVR_COMPONENTS_MAX_VOXELS voxels" in lib.svr_last_error().decode()
        assert call(cp=params(use_box=1, box_off=(0, 0, 0), box_shape=(1025, 1024, 1024)), h=other) == -1
    finally:
        N.check(lib.svr_destroy(other), "svr_destroy")
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((ids == -7).all()) and bool((records == -7).all())
    # the control cases run: too small a capacity writes the header alone; NULL arrays with capacity 0 are the count-only call
    assert call(params(selected=None, selected_count=0)) == 0
    torch.cuda.synchronize()
    assert int(header[0]) > 4 and header[2:4].tolist() == [0, 0] and bool((ids == -7).all()) and bool((records == -7).all())
    assert call(null=("ids", "records"), ids_cap=0, rec_cap=0) == 0
    assert call(params(mode=N.COMPONENTS_LEVEL, level=float("inf"), selected=None, selected_count=0)) == 0
    assert call(params(box_shape=(4, -1, 4))) == 0                      # use_box == 0 makes the box irrelevant
    torch.cuda.synchronize()
