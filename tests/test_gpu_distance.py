"""GPU: svr_distance (include/svr.h) == the numpy restatement tests/distance_twin.py, which reads the same window through
svr_read_region: the squared distances and all 16 words of the header are equal exactly, in every case.  The scene
(tests/components_scenes.py): a ring of 72 x 16 x 40 voxels (LOD 1: 36 x 12 x 20) whose window wraps on all three axes,
objects across each seam and across the corner where the seams meet; u8, u16 and float32 rings (NaN and infinities
planted); a volume without label rings; boxes of 1, 3, 4, 5 and 65 voxels along x at every alignment, one voxel thick
on every axis; a box without a source; a solid 128 x 64 x 64 volume whose few sources sit in one corner, so that most
nearest sources lie further away than any tile is wide; capacities; reproducibility; two streams; ordering behind
uploads; the Python surface; every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from components_scenes import HIGH, LEVEL, spec_of
from distance_twin import FAR, count_only, distance_twin
from sub_volume_renderer_amd import Roi, _native as N, testing

pytestmark = pytest.mark.gpu
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


def c_distance(vol, lod, *, box=None, level=None, selected=None, ignore_zero=False, invert=False, border=False, cap=None, stream=None):
    """One svr_distance call through the C ABI into a pattern-filled array of the given capacity (None: NULL and 0)
    -> (header as 16 Python ints, d2 i32 [cap] or None)."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    dp = N.DistanceParams(lod=lod, ignore_zero=int(ignore_zero), invert=int(invert), border=int(border))
    if box is not None:
        dp.use_box = 1
        dp.box_off[:], dp.box_shape[:] = box
    sel = None
    if level is not None:
        dp.mode, dp.level = N.COMPONENTS_LEVEL, level
    else:
        dp.mode = N.COMPONENTS_LABELS
        if selected is not None:
            sel = torch.from_numpy(np.unique(np.asarray(selected, np.uint32)).view(np.int32)).to(dev)
            dp.selected, dp.selected_count = sel.data_ptr(), sel.numel()
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    d2 = None if cap is None else torch.full((cap,), FILL, dtype=torch.int32, device=dev)
    do = N.DistanceOutputs(None if d2 is None else d2.data_ptr(), cap or 0, header.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    N.check(N.lib().svr_distance(handle, C.byref(dp), C.byref(do), C.c_void_p(s)), "svr_distance")
    torch.cuda.synchronize()
    return [int(v) for v in header.cpu().numpy().view(np.uint64)], None if d2 is None else d2.cpu().numpy()


def hold(vol, lod, what, *, window=None, twin=None, **mode):
    """Count, then emit into a capacity of a few elements more, and hold both to the twin (``twin``: its result where the
    caller has it already).  -> the twin's result."""
    off, shape, ring, dens, labs = window or window_of(vol, lod)
    twin = twin or distance_twin(off, dens, labs, **mode)
    want = twin["header"]
    head, _ = c_distance(vol, lod, **mode)
    assert head == count_only(want), (what, "count", head, want)
    head, d2 = c_distance(vol, lod, cap=want[2] + 3, **mode)
    assert head == want, (what, head, want)
    assert np.array_equal(d2[:want[2]], twin["d2"].reshape(-1)), (what, "d2", int((d2[:want[2]] != twin["d2"].reshape(-1)).sum()))
    assert (d2[want[2]:] == FILL).all(), (what, "beyond the end")
    return twin


def test_the_window_wraps_on_all_three_axes():
    for kind in ("u8", "f32"):
        vol = scene_of(kind)
        for lod in (0, 1):
            off, shape, ring, dens, labs = window_of(vol, lod)
            assert ring == ((40, 16, 72) if lod == 0 else (20, 12, 36))
            for a in range(3):
                assert off[a] % ring[2 - a] + shape[a] > ring[2 - a], (lod, a, off, shape)
    labs = window_of(scene_of("u8"), 0)[4]
    assert int((labs == 0xFFFFFFF0).sum()) > 30 and int((labs == 1).sum()) > 300
    dens = window_of(scene_of("f32"), 0)[3]
    assert np.isnan(dens).any() and np.isposinf(dens).any() and np.isneginf(dens).any()


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_level_mode(kind):
    vol = scene_of(kind)
    for lod in (0, 1):
        shape = window_of(vol, lod)[1]
        for name, level in (("level", LEVEL[kind]), ("high", HIGH[kind])):
            for border in (False, True):
                for invert in (False, True):
                    twin = hold(vol, lod, (kind, lod, name, border, invert), level=level, border=border, invert=invert)
                    head = twin["header"]
                    assert head[0] == (int(np.prod(shape)) - head[1] if invert else head[1]) and head[15] == 0 and head[3] >= 1
                    if name == "level":
                        assert 0.3 < head[1] / float(np.prod(shape)) < 0.7
                    elif invert:
                        assert head[3] > 16                            # few voxels reach HIGH: the others lie far from them
    if kind == "f32":
        for level in (-np.inf, np.inf, 3e38, -25.0):
            for border in (False, True):
                hold(vol, 0, (kind, "level", level, border), level=float(level), border=border)
                hold(vol, 0, (kind, "level", level, "inverted"), level=float(level), invert=True)


def test_label_modes():
    vol = scene_of("u8")
    for lod in (0, 1):
        shape = window_of(vol, lod)[1]
        voxels = int(np.prod(shape))
        for border in (False, True):
            for invert in (False, True):
                what = (lod, border, invert)
                no_zero = hold(vol, lod, (*what, "every label but 0"), ignore_zero=True, border=border, invert=invert)
                assert no_zero["header"][13] > 0 and no_zero["header"][1] + no_zero["header"][13] == voxels
                picked = hold(vol, lod, (*what, "selected"), selected=[1, 2, 3, 0xFFFFFFF0, 77], border=border, invert=invert)
                assert 0 < picked["header"][1] < voxels // 4 and picked["header"][13] == 0
                hold(vol, lod, (*what, "near 2^32 alone"), selected=[0xFFFFFFF0], border=border, invert=invert)
                hold(vol, lod, (*what, "selected with zero dropped"), selected=[0, 9], ignore_zero=True, border=border, invert=invert)
        # background=True: every voxel is inside, so nothing is a source but the border
        solid = hold(vol, lod, (lod, "background"), border=False)
        assert solid["header"][:4] == [voxels, voxels, voxels, 0] and solid["header"][14:] == [0, voxels] and (solid["d2"] == FAR).all()
        faces = hold(vol, lod, (lod, "background, border"), border=True)
        assert faces["header"][3] == ((min(shape) + 1) // 2) ** 2 and faces["header"][15] == 0
        nothing = hold(vol, lod, (lod, "background, inverted"), invert=True)
        assert nothing["header"][:4] == [0, voxels, voxels, 0] and not nothing["d2"].any()
        none = hold(vol, lod, (lod, "none inside, inverted"), selected=[123456], invert=True, border=True)
        assert none["header"][:2] == [voxels, 0] and none["header"][15] == voxels


def test_without_label_rings():
    vol = scene_of("nolabels")
    assert not vol._rings.labels
    for lod in (0, 1):
        off, shape, ring, dens, labs = window_of(vol, lod)
        voxels = int(np.prod(shape))
        assert labs is None
        assert hold(vol, lod, "every label reads 0", border=False)["header"][15] == voxels
        dropped = hold(vol, lod, "and is dropped", ignore_zero=True, border=True)
        assert dropped["header"][:2] == [0, 0] and dropped["header"][13] == voxels
        assert hold(vol, lod, "{5}", selected=[5], invert=True)["header"][15] == voxels
        hold(vol, lod, "level", level=LEVEL["u8"], border=True)


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
            hold(vol, 0, ("row", nx, start), box=box, border=bool(start % 2), invert=bool(nx % 2 == 0 and start == 2), **mode)
    # rows of 29 .. 35 voxels at every alignment: one and two words of source bits
    for nx in (29, 30, 31, 32, 33, 35):
        for start in (0, 1, 2, 3):
            hold(vol, 0, ("words", nx, start), box=((off[0] + start, off[1] + 3, off[2] + 20), (nx, 2, 3)), level=HIGH["u8"], invert=True)
    # one voxel thick on each axis in turn
    for name, n in (("x", (1, 11, 21)), ("y", (41, 1, 21)), ("z", (41, 11, 1)), ("a row", (41, 1, 1)), ("a column", (1, 1, 21))):
        for border in (False, True):
            hold(vol, 0, ("thin", name, border), box=((off[0] + 30, off[1] + 2, off[2] + 11), n), level=LEVEL["u8"], border=border)
        hold(vol, 0, ("thin, labels", name), box=((off[0] + 30, off[1] + 2, off[2] + 11), n), ignore_zero=True, invert=True)
    hold(vol, 0, "partly outside", box=((off[0] - 5, off[1] + 2, off[2] + shape[2] - 6), (20, shape[1] + 9, 30)), level=LEVEL["u8"], border=True)
    for border in (False, True):
        one = hold(vol, 0, "one voxel", box=((off[0] + 7, off[1] + 3, off[2] + 9), (1, 1, 1)), border=border)
        assert one["header"][:4] == [1, 1, 1, int(border)] and one["header"][14:] == [0, 1 - int(border)]
    for name, box in (("misses", ((off[0] + shape[0] + 4, off[1], off[2]), (4, 4, 4))), ("empty shape", ((off[0] + 4, off[1] + 2, off[2] + 2), (0, 5, 5)))):
        twin = hold(vol, 0, name, box=box, level=1.0, border=True)
        assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7:] == [0] * 9
    # a window of None
    spec = spec_of("u8")
    spec.centers = []
    bare = testing.build(spec).volume
    try:
        head, d2 = c_distance(bare, 0, level=1.0, cap=4, border=True)
        assert head == [0] * 16 and (d2 == FILL).all()
        assert distance_twin((0, 0, 0), None, None, level=1.0)["header"] == head
    finally:
        bare.close()


def test_a_box_with_no_source_where_the_three_seams_meet():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    box = ((71, 31, 39), (3, 3, 3))                                     # around (72, 32, 40), inside the ball of label 1
    for a, seam in enumerate((72, 32, 40)):                             # the box lies on both sides of every seam
        assert seam % ring[2 - a] == 0 and off[a] < seam - 1 and seam + 1 < off[a] + shape[a]
    cut = tuple(slice(box[0][a] - off[a], box[0][a] - off[a] + 3) for a in (2, 1, 0))
    assert (labs[cut] == 1).all()
    far = hold(vol, 0, "no source", box=box, selected=[1], border=False)
    assert far["header"][:4] == [27, 27, 27, 0] and far["header"][14:] == [0, 27] and (far["d2"] == FAR).all()
    faces = hold(vol, 0, "no source, border", box=box, selected=[1], border=True)
    want = np.ones((3, 3, 3), np.int32)
    want[1, 1, 1] = 4
    assert np.array_equal(faces["d2"], want) and faces["header"][:4] == [27, 27, 27, 4] and faces["header"][14:] == [13, 0]
    inverted = hold(vol, 0, "no target", box=box, selected=[1], invert=True)
    assert inverted["header"][:4] == [0, 27, 27, 0] and not inverted["d2"].any()


SOURCES = [(0, 0, 0), (3, 1, 2), (1, 5, 0), (2, 2, 7), (6, 0, 1)]        # (x, y, z): the only voxels of label 0


def deep_spec():
    """A 128 x 64 x 64 volume (x, y, z extents) of label 1, the whole of it resident, but for SOURCES near one corner."""
    lab = np.ones((64, 64, 128), np.uint32)
    for x, y, z in SOURCES:
        lab[z, y, x] = 0
    d = (lab * 200).astype(np.uint8)
    spec = testing.synthetic_spec(64, 32, 32, pairs=[(d, lab)], chunk_shapes=[(8, 8, 8)], ring_shapes=[(8, 8, 16)])
    spec.centers = [((63.5, 31.5, 31.5), None)]
    return spec


def test_deep_and_long_columns():
    vol = testing.build(deep_spec()).volume
    try:
        window = window_of(vol, 0)
        assert window[0] == [0, 0, 0] and window[1] == [128, 64, 64]
        z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(128), indexing="ij")
        direct = np.minimum.reduce([(x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2 for sx, sy, sz in SOURCES])     # what it must be
        face = np.minimum.reduce([x + 1, 128 - x, y + 1, 64 - y, z + 1, 64 - z]) ** 2
        assert (direct > 64 ** 2).mean() > 0.5                          # most nearest sources lie more than 64 voxels away
        twins = {border: distance_twin(window[0], window[3], window[4], selected=[1], border=border) for border in (False, True)}
        assert np.array_equal(twins[False]["d2"], direct) and np.array_equal(twins[True]["d2"], np.minimum(direct, face))
        head = twins[False]["header"]
        # the far corner is the deepest voxel, 121 or more voxels from the sources on x alone
        assert head[3] == int(direct[63, 63, 127]) == int(direct.max()) > 121 ** 2 and head[14] == 128 * 64 * 64 - 1
        assert head[:3] == [128 * 64 * 64 - len(SOURCES)] * 2 + [128 * 64 * 64] and head[15] == 0
        # with the border the faces win: the deepest voxels form a line along x in the middle, and its first voxel counts
        assert twins[True]["header"][3] == 32 ** 2 and twins[True]["header"][14] == (31 * 64 + 31) * 128 + 31
        for mode in (dict(selected=[1]), dict(level=100.0)):             # the same inside set either way, and the same header
            for border in (False, True):
                hold(vol, 0, ("deep", tuple(mode), border), window=window, twin=twins[border], border=border, **mode)
        inverted = hold(vol, 0, "deep, inverted", window=window, selected=[1], invert=True)
        assert inverted["header"][:2] == [len(SOURCES), 128 * 64 * 64 - len(SOURCES)] and inverted["header"][3] == 1
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_capacities():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    for mode in (dict(selected=[1, 2, 3, 9], border=True), dict(level=LEVEL["u8"], invert=True)):
        twin = distance_twin(off, dens, labs, **mode)
        want = twin["header"]
        n = want[2]
        assert n == int(np.prod(shape)) and want[3] > 0
        head, d2 = c_distance(vol, 0, **mode)                              # the count-only call
        assert head == count_only(want) and d2 is None
        for cap in (1, n - 1):                                             # too small: the array is not touched
            head, d2 = c_distance(vol, 0, cap=cap, **mode)
            assert head == count_only(want) and (d2 == FILL).all()
        head, d2 = c_distance(vol, 0, cap=n, **mode)
        assert head == want and np.array_equal(d2, twin["d2"].reshape(-1))


def test_two_calls_and_two_streams_give_identical_bytes():
    vol = scene_of("u8")
    dev = torch.device("cuda", vol._rings.device)
    off, shape, ring, dens, labs = window_of(vol, 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for mode in (dict(level=LEVEL["u8"], border=True), dict(ignore_zero=True, invert=True)):
        twin = hold(vol, 0, "first", **mode)
        n = twin["header"][2]
        runs = [c_distance(vol, 0, cap=n, **mode) for _ in range(2)]
        runs += [c_distance(vol, 0, cap=n, stream=s.cuda_stream, **mode) for s in streams]
        for head, d2 in runs:
            assert head == twin["header"] and d2.tobytes() == twin["d2"].tobytes()
    # two calls in flight on two streams at once: the second is ordered behind the first in the shared scratch
    handle = vol.prepare()
    outs = []
    torch.cuda.synchronize()
    for s, level in zip(streams, (LEVEL["u8"], HIGH["u8"])):
        twin = distance_twin(off, dens, labs, level=level, invert=level == HIGH["u8"])
        dp = N.DistanceParams(lod=0, mode=N.COMPONENTS_LEVEL, level=level, invert=int(level == HIGH["u8"]))
        header = torch.full((16,), -7, dtype=torch.int64, device=dev)
        d2 = torch.zeros(twin["header"][2], dtype=torch.int32, device=dev)
        outs.append((twin, header, d2))
        torch.cuda.synchronize()
        do = N.DistanceOutputs(d2.data_ptr(), d2.numel(), header.data_ptr())
        N.check(N.lib().svr_distance(handle, C.byref(dp), C.byref(do), C.c_void_p(s.cuda_stream)), "svr_distance")
    torch.cuda.synchronize()
    for twin, header, d2 in outs:
        assert [int(v) for v in header.cpu().numpy().view(np.uint64)] == twin["header"]
        assert d2.cpu().numpy().tobytes() == twin["d2"].tobytes()


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
            n = int(np.prod(window_of(vol, 0)[1]))
            got = [c_distance(vol, 0, selected=[1, 2], cap=n), c_distance(vol, 0, level=100.0, border=True, cap=n)]
            window = window_of(vol, 0, fresh=True)
            for (head, d2), mode in zip(got, (dict(selected=[1, 2]), dict(level=100.0, border=True))):
                twin = distance_twin(window[0], window[3], window[4], **mode)
                assert head == twin["header"] and np.array_equal(d2, twin["d2"].reshape(-1)), (step, mode)
            hold(vol, 0, ("after upload", step), window=window, ignore_zero=True, border=True)
        N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
        N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
        n = int(np.prod(window_of(vol, 0)[1]))
        assert c_distance(vol, 0, level=1.0)[0][:2] == [0, 0]
        assert c_distance(vol, 0, level=1.0, invert=True, cap=n)[0][:4] == [n, 0, n, 0]
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_python_surface():
    vol = scene_of("u8")
    vol.world.scale = (1.5, 0.5, 2.0)
    vol.world.position = (3.0, -2.0, 7.0)
    try:
        for lod, kw, mode in ((0, dict(level=LEVEL["u8"]), dict(level=LEVEL["u8"], border=True)),
                              (0, dict(level=HIGH["u8"], invert=True, border=False), dict(level=HIGH["u8"], invert=True)),
                              (1, dict(labels=[9, 1, 9], border=False), dict(selected=[1, 9], ignore_zero=True)),
                              (0, dict(background=True, box=((20, 26, 50), (44, 36, 90))), dict(border=True))):
            off, shape, ring, dens, labs = window_of(vol, lod)
            if "box" in kw:
                b, e = kw["box"]
                mode["box"] = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))               # LOD 0: scale 1
            twin = distance_twin(off, dens, labs, **mode)
            got = vol.distance(lod=lod, **kw)
            head = twin["header"]
            assert got.squared.is_cuda and got.squared.dtype == torch.int32 and tuple(got.squared.shape) == twin["d2"].shape
            assert np.array_equal(got.squared.cpu().numpy(), twin["d2"])
            assert (got.targets, got.inside_voxels, got.far_voxels, got.max_squared, got.background, got.lod) == \
                (head[0], head[1], head[15], head[3], head[13], lod)
            assert tuple(got.begin) == tuple(head[7:10][::-1]) and tuple(got.offset) == tuple(off[::-1])
            n = head[10:13]
            deepest = (head[9] + head[14] // (n[0] * n[1]), head[8] + head[14] // n[0] % n[1], head[7] + head[14] % n[0])
            assert tuple(got.deepest) == deepest and head[3] > 0 and got.radius() == float(np.sqrt(head[3]))
            scale = np.array(vol.wrapping_buffers[lod].scale_factor, np.float64)
            data = (np.array(deepest[::-1], np.float64) + 0.5) / scale[::-1] - 0.5
            world = data * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0])
            assert np.allclose(got.deepest_position(), world, rtol=0, atol=1e-9)
            assert got.at(got.deepest_position()) == head[3] and got.at((-1e5, 0.0, 0.0)) == 0
            d2 = twin["d2"].astype(np.int64)
            assert got.distance().is_cuda and np.array_equal(got.distance().cpu().numpy(), np.sqrt(d2).astype(np.float32))
            assert np.array_equal(got.eroded(2).cpu().numpy(), d2 > 4) and np.array_equal(got.within(1.5).cpu().numpy(), (d2 > 0) & (d2 <= 2))
        # signed: the two calls, positive inside and negative outside
        off, shape, ring, dens, labs = window_of(vol, 0)
        for border in (True, False):
            inner = distance_twin(off, dens, labs, level=LEVEL["u8"], border=border)
            outer = distance_twin(off, dens, labs, level=LEVEL["u8"], invert=True)
            got = vol.distance(level=LEVEL["u8"], signed=True, border=border, invert=border)              # invert is not read
            assert np.array_equal(got.squared.cpu().numpy(), inner["d2"] - outer["d2"]) and got.squared.dtype == torch.int32
            assert (got.targets, got.max_squared, got.far_voxels) == (inner["header"][0], inner["header"][3], 0)
        solid = vol.distance(background=True, signed=True, border=False)                                   # a FAR stays FAR, on either side
        assert bool((solid.squared == FAR).all()) and solid.far_voxels == solid.targets == int(np.prod(shape)) and solid.max_squared == 0
        assert bool(torch.isinf(solid.distance()).all()) and tuple(solid.deepest) == tuple(solid.begin)
        none = vol.distance(labels=[123456], signed=True)
        assert bool((none.squared == -FAR).all()) and none.targets == 0 and none.far_voxels == int(np.prod(shape))
        empty = vol.distance(level=1.0, box=((0, 0, 0), (4, 4, 4)))                                       # misses the window
        assert empty.squared.numel() == 0 and empty.targets == 0 and empty.max_squared == 0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        again = vol.distance(labels=[1], stream=side.cuda_stream)
        side.synchronize()
        want = distance_twin(off, dens, labs, selected=[1], border=True)
        assert np.array_equal(again.squared.cpu().numpy(), want["d2"]) and again.max_squared == want["header"][3]
    finally:
        vol.world.scale = (1.0, 1.0, 1.0)
        vol.world.position = (0.0, 0.0, 0.0)


def test_refusals_enqueue_nothing():
    vol = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    d2 = torch.full((64,), -7, dtype=torch.int32, device=dev)
    sel = torch.tensor([1, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        dp = N.DistanceParams(lod=0, mode=N.COMPONENTS_LABELS, selected=sel.data_ptr(), selected_count=2)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(dp, k)[:] = v
            else:
                setattr(dp, k, v)
        return dp

    def call(dp=None, h=handle, null=(), cap=64):
        dp = dp or params()
        do = N.DistanceOutputs(None if "d2" in null else d2.data_ptr(), cap, None if "header" in null else header.data_ptr())
        return lib.svr_distance(h, None if "params" in null else C.byref(dp), None if "out" in null else C.byref(do), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("header",)), "null argument"),
        (dict(dp=params(lod=-1)), "lod out of range"), (dict(dp=params(lod=2)), "lod out of range"),
        (dict(dp=params(mode=2)), "unknown mode"), (dict(dp=params(mode=-1)), "unknown mode"),
        (dict(dp=params(mode=N.COMPONENTS_LEVEL, level=float("nan"))), "level must not be NaN"),
        (dict(dp=params(selected=None)), "NULL selected pointer"),
        (dict(dp=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(null=("d2",)), "NULL d2"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((d2 == -7).all())                                           # nothing was enqueued
    # the two limits, on contexts of their own, whose memory no kernel touches: u8 rings without labels
    for ring, shapes, msg in (((1032, 1024, 1024), [None, (1025, 1024, 1024)], "more than SVR_DISTANCE_MAX_VOXELS voxels"),
                              ((16392, 8, 8), [None, (16385, 1, 1)], "an extent of more than SVR_DISTANCE_MAX_EXTENT voxels")):
        desc = (N.LodDesc * 1)()
        desc[0].ring_dims[:] = ring
        desc[0].density_storage, desc[0].no_labels, desc[0].blocked_twin = N.SVR_U8, 1, 0
        other = C.c_void_p()
        N.check(lib.svr_create(vol._rings.device, 1, desc, C.byref(other)), "svr_create")
        try:
            st = N.LodState()
            st.offset[:], st.shape[:], st.scale[:] = (0, 0, 0), ring, (1.0, 1.0, 1.0)
            N.check(lib.svr_set_lod_state(other, 0, C.byref(st)), "svr_set_lod_state")
            for shape in shapes:
                dp = params(selected=None, selected_count=0) if shape is None else params(use_box=1, box_off=(0, 0, 0), box_shape=shape)
                assert call(dp=dp, h=other) == -1 and msg in lib.svr_last_error().decode(), (ring, shape)
                assert call(dp=dp, h=other, null=("d2",), cap=0) == -1                                     # the count-only call too
        finally:
            N.check(lib.svr_destroy(other), "svr_destroy")
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((d2 == -7).all())
    # the control cases run: too small a capacity writes the header alone; a NULL array with capacity 0 is the count-only call
    assert call(params(selected=None, selected_count=0)) == 0
    torch.cuda.synchronize()
    assert int(header[0]) > 4 and header[2:4].tolist() == [0, 0] and header[14:].tolist() == [0, 0] and bool((d2 == -7).all())
    assert call(null=("d2",), cap=0) == 0
    assert call(params(mode=N.COMPONENTS_LEVEL, level=float("inf"), selected=None, selected_count=0)) == 0
    assert call(params(box_shape=(4, -1, 4))) == 0                      # use_box == 0 makes the box irrelevant
    torch.cuda.synchronize()
