"""GPU: svr_nearest (include/svr.h) == the numpy restatement tests/nearest_twin.py, which reads the same window through
svr_read_region: d2, index, label and all 16 words of the header are equal exactly, in every case.  The scenes are those of
tests/test_gpu_distance.py (tests/components_scenes.py): the ring of 72 x 16 x 40 voxels whose window wraps on all three
axes, and LOD 1; u8, u16 and float32 rings; a volume without label rings; boxes of 1, 3, 4, 5 and 65 voxels along x at
every alignment, one voxel thick on every axis; a box without a source; the planted checkerboard, where more than half
of the targets have several nearest sources and the tie rule decides; a solid 128 x 64 x 64 volume whose few sources sit
in one corner; agreement with svr_distance; capacities; reproducibility; two streams, and svr_distance and svr_nearest in
the scratch they share; ordering behind uploads; the Python surface; every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from components_scenes import CHECKER, HIGH, LEVEL, PLANTED, spec_of
from distance_twin import FAR, count_only
from nearest_twin import brute_force, expanded, nearest_twin, tied
from sub_volume_renderer_amd import NearestField, Roi, _native as N, testing

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


def params_of(lod, *, box=None, level=None, selected=None, ignore_zero=False, invert=False, dev=None, cls=None, **more):
    """The params struct (``cls``: NearestParams, or DistanceParams with ``more``) and the uploaded id list, which must live
    as long as the call."""
    p = (cls or N.NearestParams)(lod=lod, ignore_zero=int(ignore_zero), invert=int(invert), **more)
    if box is not None:
        p.use_box = 1
        p.box_off[:], p.box_shape[:] = box
    sel = None
    if level is not None:
        p.mode, p.level = N.COMPONENTS_LEVEL, level
    else:
        p.mode = N.COMPONENTS_LABELS
        if selected is not None:
            sel = torch.from_numpy(np.unique(np.asarray(selected, np.uint32)).view(np.int32)).to(dev)
            p.selected, p.selected_count = sel.data_ptr(), sel.numel()
    return p, sel


def c_nearest(vol, lod, *, cap=None, stream=None, with_label=True, **mode):
    """One svr_nearest call through the C ABI into pattern-filled arrays of the given capacity (None: NULL and 0)
    -> (header as 16 Python ints, d2, index, label as numpy [cap], or None each)."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    p, sel = params_of(lod, dev=dev, **mode)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    arrays = [None if cap is None or (k == 2 and not with_label) else torch.full((cap,), FILL, dtype=torch.int32, device=dev) for k in range(3)]
    out = N.NearestOutputs(*[None if t is None else t.data_ptr() for t in arrays], cap or 0, header.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    N.check(N.lib().svr_nearest(handle, C.byref(p), C.byref(out), C.c_void_p(s)), "svr_nearest")
    torch.cuda.synchronize()
    d2, index, label = [None if t is None else t.cpu().numpy() for t in arrays]
    return [int(v) for v in header.cpu().numpy().view(np.uint64)], d2, index, None if label is None else label.view(np.uint32)


def c_distance(vol, lod, *, cap, stream=None, **mode):
    """svr_distance with border = 0 on the same parameters -> (header, d2)."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    p, sel = params_of(lod, dev=dev, cls=N.DistanceParams, border=0, **mode)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    d2 = torch.full((cap,), FILL, dtype=torch.int32, device=dev)
    out = N.DistanceOutputs(d2.data_ptr(), cap, header.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    N.check(N.lib().svr_distance(handle, C.byref(p), C.byref(out), C.c_void_p(s)), "svr_distance")
    torch.cuda.synchronize()
    return [int(v) for v in header.cpu().numpy().view(np.uint64)], d2.cpu().numpy()


def same(what, got, twin, n):
    head, d2, index, label = got
    assert head == twin["header"], (what, head, twin["header"])
    for name, arr in (("d2", d2), ("index", index), ("label", label)):
        want = twin[name].reshape(-1)
        assert np.array_equal(arr[:n], want), (what, name, int((arr[:n] != want).sum()))
        assert (arr[n:].view(np.uint32) == FILL).all(), (what, name, "beyond the end")


def hold(vol, lod, what, *, window=None, twin=None, **mode):
    """Count, then emit into a capacity of a few elements more, and hold both to the twin (``twin``: its result where the
    caller has it already).  -> the twin's result."""
    off, shape, ring, dens, labs = window or window_of(vol, lod)
    twin = twin or nearest_twin(off, dens, labs, **mode)
    want = twin["header"]
    head = c_nearest(vol, lod, **mode)[0]
    assert head == count_only(want), (what, "count", head, want)
    same(what, c_nearest(vol, lod, cap=want[2] + 3, **mode), twin, want[2])
    return twin


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_level_mode(kind):
    vol = scene_of(kind)
    for lod in (0, 1):
        off, shape, ring, dens, labs = window_of(vol, lod)
        for a in range(3):
            assert off[a] % ring[2 - a] + shape[a] > ring[2 - a], (lod, a)              # the window wraps on every axis
        for name, level in (("level", LEVEL[kind]), ("high", HIGH[kind])):
            for invert in (False, True):
                twin = hold(vol, lod, (kind, lod, name, invert), level=level, invert=invert)
                head = twin["header"]
                assert head[15] == 0 and head[3] >= 1 and (twin["index"] >= 0).all()
                if name == "high" and invert:
                    assert head[3] > 16                                 # few voxels reach HIGH: the others lie far from their owners
    if kind == "f32":
        for level in (-np.inf, np.inf):
            hold(vol, 0, (kind, "level", level), level=float(level))
            hold(vol, 0, (kind, "level", level, "inverted"), level=float(level), invert=True)


def test_label_modes():
    vol = scene_of("u8")
    for lod in (0, 1):
        shape = window_of(vol, lod)[1]
        labs = window_of(vol, lod)[4]
        voxels = int(np.prod(shape))
        for invert in (False, True):
            every = hold(vol, lod, (lod, invert, "every label"), invert=invert)
            assert every["header"][15] == (0 if invert else voxels)
            no_zero = hold(vol, lod, (lod, invert, "every label but 0"), ignore_zero=True, invert=invert)
            assert no_zero["header"][13] > 0
            hold(vol, lod, (lod, invert, "selected"), selected=[1, 2, 3, 0xFFFFFFF0, 77], invert=invert)
            hold(vol, lod, (lod, invert, "selected with zero dropped"), selected=[0, 9], ignore_zero=True, invert=invert)
        # the grown objects: every label-0 voxel takes the label of the nearest object, an object voxel keeps its own
        grown = hold(vol, lod, (lod, "grown"), ignore_zero=True, invert=True)
        assert np.array_equal(grown["label"][labs != 0], labs[labs != 0]) and (grown["label"] != 0).all()
        far_label = hold(vol, lod, (lod, "near 2^32 alone"), selected=[0xFFFFFFF0], invert=True)
        if lod == 0:
            assert (far_label["label"] == 0xFFFFFFF0).all() and (grown["label"] == 0xFFFFFFF0).sum() >= (labs == 0xFFFFFFF0).sum() > 30
        none = hold(vol, lod, (lod, "none inside, inverted"), selected=[123456], invert=True)
        assert none["header"][15] == voxels and (none["index"] == -1).all() and not none["label"].any() and (none["d2"] == FAR).all()


def test_without_label_rings():
    vol = scene_of("nolabels")
    assert not vol._rings.labels
    for lod in (0, 1):
        assert window_of(vol, lod)[4] is None
        for mode in (dict(level=LEVEL["u8"]), dict(level=HIGH["u8"], invert=True), dict(), dict(selected=[5], invert=True), dict(ignore_zero=True, invert=True)):
            assert not hold(vol, lod, ("no labels", lod, tuple(mode)), **mode)["label"].any()


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
            hold(vol, 0, ("row", nx, start), box=box, invert=bool(nx % 2 == 0 or start == 2), **mode)
    for nx in (31, 32, 33):                                             # one and two words of source bits
        for start in (0, 1, 2, 3):
            hold(vol, 0, ("words", nx, start), box=((off[0] + start, off[1] + 3, off[2] + 20), (nx, 2, 3)), level=HIGH["u8"], invert=True)
    for name, n in (("x", (1, 11, 21)), ("y", (41, 1, 21)), ("z", (41, 11, 1)), ("a row", (41, 1, 1)), ("a column", (1, 1, 21)), ("one voxel", (1, 1, 1))):
        hold(vol, 0, ("thin", name), box=((off[0] + 30, off[1] + 2, off[2] + 11), n), level=LEVEL["u8"])
        hold(vol, 0, ("thin, labels", name), box=((off[0] + 30, off[1] + 2, off[2] + 11), n), ignore_zero=True, invert=True)
    hold(vol, 0, "partly outside", box=((off[0] - 5, off[1] + 2, off[2] + shape[2] - 6), (20, shape[1] + 9, 30)), ignore_zero=True, invert=True)
    for name, box in (("misses", ((off[0] + shape[0] + 4, off[1], off[2]), (4, 4, 4))), ("empty shape", ((off[0] + 4, off[1] + 2, off[2] + 2), (0, 5, 5)))):
        twin = hold(vol, 0, name, box=box, level=1.0)
        assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7:] == [0] * 9


def test_a_box_with_no_source_where_the_three_seams_meet():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    box = ((71, 31, 39), (3, 3, 3))                                     # around (72, 32, 40), inside the ball of label 1
    cut = tuple(slice(box[0][a] - off[a], box[0][a] - off[a] + 3) for a in (2, 1, 0))
    assert (labs[cut] == 1).all()
    far = hold(vol, 0, "no source", box=box, selected=[1])
    assert far["header"][:4] == [27, 27, 27, 0] and far["header"][14:] == [0, 27]
    assert (far["d2"] == FAR).all() and (far["index"] == -1).all() and not far["label"].any()
    own = hold(vol, 0, "no target", box=box, selected=[1], invert=True)
    assert np.array_equal(own["index"].reshape(-1), np.arange(27)) and (own["label"] == 1).all() and not own["d2"].any()


def test_the_tie_rule_decides_on_the_checkerboard():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    mode = dict(box=CHECKER, selected=[PLANTED["checker"]], invert=True)
    twin = hold(vol, 0, "checkerboard", **mode)
    lo, n = twin["header"][7:10], twin["header"][10:13]
    assert min(n) >= 4                                                  # the window holds enough of the planted box
    cut = labs[tuple(slice(lo[a] - off[a], lo[a] - off[a] + n[a]) for a in (2, 1, 0))]
    source = cut == PLANTED["checker"]
    several = tied(source)
    assert several.sum() * 2 > (~source).sum() > 50                     # more than half of the targets have two or more nearest sources
    d2, index = brute_force(source)
    assert np.array_equal(twin["index"], index) and np.array_equal(twin["d2"], d2)
    assert (twin["label"] == PLANTED["checker"]).all()


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
        order = sorted(SOURCES, key=lambda s: (s[2] * 64 + s[1]) * 128 + s[0])          # ascending dense index: argmin keeps the first
        each = np.stack([(x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2 for sx, sy, sz in order])
        direct = each.min(axis=0)
        owner = np.array([(sz * 64 + sy) * 128 + sx for sx, sy, sz in order])[each.argmin(axis=0)]
        assert (direct > 64 ** 2).mean() > 0.5                          # most nearest sources lie more than 64 voxels away
        twin = nearest_twin(window[0], window[3], window[4], selected=[1])
        assert np.array_equal(twin["d2"], direct) and np.array_equal(twin["index"], owner) and not twin["label"].any()
        for mode in (dict(selected=[1]), dict(level=100.0)):            # the same inside set either way
            hold(vol, 0, ("deep", tuple(mode)), window=window, twin=twin, **mode)
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_d2_and_header_are_svr_distances_bytes():
    vol = scene_of("u8")
    n = int(np.prod(window_of(vol, 0)[1]))
    for mode in (dict(level=LEVEL["u8"]), dict(level=HIGH["u8"], invert=True), dict(ignore_zero=True, invert=True), dict(selected=[1, 9]),
                 dict(selected=[123456], invert=True), dict(level=LEVEL["u8"], box=((60, 26, 30), (33, 7, 9)))):
        head, d2, index, label = c_nearest(vol, 0, cap=n, **mode)
        want_head, want = c_distance(vol, 0, cap=n, **mode)
        assert head == want_head and d2.tobytes() == want.tobytes(), mode
        assert c_nearest(vol, 0, **mode)[0] == count_only(want_head)


def test_capacities_and_a_null_label():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    for mode in (dict(ignore_zero=True, invert=True), dict(level=LEVEL["u8"])):
        twin = nearest_twin(off, dens, labs, **mode)
        want = twin["header"]
        n = want[2]
        assert n == int(np.prod(shape)) and want[3] > 0
        head, d2, index, label = c_nearest(vol, 0, **mode)                 # the count-only call
        assert head == count_only(want) and d2 is None and index is None and label is None
        for cap in (1, n - 1):                                             # too small: no array is touched
            head, d2, index, label = c_nearest(vol, 0, cap=cap, **mode)
            assert head == count_only(want)
            assert (d2.view(np.uint32) == FILL).all() and (index.view(np.uint32) == FILL).all() and (label == FILL).all()
        full = c_nearest(vol, 0, cap=n, **mode)
        same(("exact", tuple(mode)), full, twin, n)
        head, d2, index, label = c_nearest(vol, 0, cap=n, with_label=False, **mode)         # a NULL label: the other two as before
        assert label is None and head == want and d2.tobytes() == full[1].tobytes() and index.tobytes() == full[2].tobytes()


def test_two_calls_and_two_streams_give_identical_bytes():
    vol = scene_of("u8")
    dev = torch.device("cuda", vol._rings.device)
    off, shape, ring, dens, labs = window_of(vol, 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    mode = dict(ignore_zero=True, invert=True)
    twin = hold(vol, 0, "first", **mode)
    n = twin["header"][2]
    runs = [c_nearest(vol, 0, cap=n, **mode) for _ in range(2)] + [c_nearest(vol, 0, cap=n, stream=s.cuda_stream, **mode) for s in streams]
    for run in runs:
        same("again", run, twin, n)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run[1:], runs[0][1:]))
    # svr_distance and svr_nearest in flight on two streams at once: the second is ordered behind the first in the scratch
    # they share, in either order
    handle = vol.prepare()
    want_near = nearest_twin(off, dens, labs, level=HIGH["u8"], invert=True)
    want_dist = nearest_twin(off, dens, labs, level=LEVEL["u8"])
    for first in ("distance", "nearest"):
        dp, _ = params_of(0, level=LEVEL["u8"], cls=N.DistanceParams, border=0)
        npar, _ = params_of(0, level=HIGH["u8"], invert=True)
        heads = [torch.full((16,), -7, dtype=torch.int64, device=dev) for _ in range(2)]
        arrays = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
        do = N.DistanceOutputs(arrays[0].data_ptr(), n, heads[0].data_ptr())
        no = N.NearestOutputs(arrays[1].data_ptr(), arrays[2].data_ptr(), arrays[3].data_ptr(), n, heads[1].data_ptr())
        torch.cuda.synchronize()
        calls = [lambda: N.check(N.lib().svr_distance(handle, C.byref(dp), C.byref(do), C.c_void_p(streams[0].cuda_stream)), "svr_distance"),
                 lambda: N.check(N.lib().svr_nearest(handle, C.byref(npar), C.byref(no), C.c_void_p(streams[1].cuda_stream)), "svr_nearest")]
        for call in (calls if first == "distance" else calls[::-1]):
            call()
        torch.cuda.synchronize()
        assert [int(v) for v in heads[0].cpu().numpy().view(np.uint64)] == want_dist["header"], first
        assert arrays[0].cpu().numpy().tobytes() == want_dist["d2"].tobytes(), first
        got = ([int(v) for v in heads[1].cpu().numpy().view(np.uint64)], arrays[1].cpu().numpy(), arrays[2].cpu().numpy(), arrays[3].cpu().numpy().view(np.uint32))
        same(("shared scratch", first), got, want_near, n)


def test_a_call_right_after_an_upload_sees_it():
    vol = testing.build(spec_of("u8")).volume
    try:
        lib, handle = N.lib(), vol.prepare()
        buf = vol.wrapping_buffers[0]
        rng = np.random.default_rng(2)
        for step in range(2):
            block_d = rng.integers(0, 256, (16, 8, 24)).astype(np.uint8)
            block_l = rng.integers(0, 3, (16, 8, 24)).astype(np.uint32) * np.uint32(7 + step)
            buf._upload(Roi((8 * step, 4, 16 * step), (16, 8, 24)), block_d, block_l)
            N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
            n = int(np.prod(window_of(vol, 0)[1]))
            got = c_nearest(vol, 0, ignore_zero=True, invert=True, cap=n)
            window = window_of(vol, 0, fresh=True)
            same(("after upload", step), got, nearest_twin(window[0], window[3], window[4], ignore_zero=True, invert=True), n)
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_python_surface():
    vol = scene_of("u8")
    vol.world.scale = (1.5, 0.5, 2.0)
    vol.world.position = (3.0, -2.0, 7.0)
    try:
        for lod, kw, mode in ((0, dict(level=LEVEL["u8"]), dict(level=LEVEL["u8"])),
                              (0, dict(invert=True), dict(ignore_zero=True, invert=True)),
                              (1, dict(labels=[9, 1, 9], invert=True, with_labels=False), dict(selected=[1, 9], ignore_zero=True, invert=True)),
                              (0, dict(background=True, labels=[0, 1], box=((20, 26, 50), (44, 36, 90))), dict(selected=[0, 1]))):
            off, shape, ring, dens, labs = window_of(vol, lod)
            if "box" in kw:
                b, e = kw["box"]
                mode["box"] = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))               # LOD 0: scale 1
            twin = nearest_twin(off, dens, labs, **mode)
            got = vol.nearest(lod=lod, **kw)
            head = twin["header"]
            assert isinstance(got, NearestField) and got.squared.is_cuda and got.index.is_cuda and got.index.dtype == torch.int32
            assert np.array_equal(got.squared.cpu().numpy(), twin["d2"]) and np.array_equal(got.index.cpu().numpy(), twin["index"])
            if kw.get("with_labels", True):
                assert got.label.is_cuda and got.label.dtype == torch.uint32 and np.array_equal(got.label.cpu().numpy(), twin["label"])
                for r in (0, 1.5, 3):
                    assert np.array_equal(got.expanded(r).cpu().numpy(), expanded(twin, r)), r
            else:
                assert got.label is None
            assert (got.targets, got.inside_voxels, got.far_voxels, got.max_squared, got.background, got.lod) == \
                (head[0], head[1], head[15], head[3], head[13], lod)
            assert tuple(got.begin) == tuple(head[7:10][::-1]) and tuple(got.offset) == tuple(off[::-1])
            nz, ny, nx = twin["d2"].shape
            i = twin["index"].astype(np.int64)
            want = np.stack([i // (ny * nx) + head[9], i // nx % ny + head[8], i % nx + head[7]], -1)
            assert np.array_equal(got.nearest_voxel().cpu().numpy(), want)
            assert np.array_equal((got.vector().cpu().numpy().astype(np.int64) ** 2).sum(-1), twin["d2"])
            # a picked point snaps to the centre of a source voxel: the deepest target's nearest source
            picked = got.deepest_position()
            there = got.nearest_position(picked)
            assert got.at(picked) == head[3] > 0 and got.at(there) == 0
            at = head[14]
            scale = np.array(vol.wrapping_buffers[lod].scale_factor, np.float64)
            data = (want.reshape(-1, 3)[at][::-1].astype(np.float64) + 0.5) / scale[::-1] - 0.5
            assert np.allclose(there, data * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0]), rtol=0, atol=1e-9)
        off, shape, ring, dens, labs = window_of(vol, 0)
        grown = nearest_twin(off, dens, labs, ignore_zero=True, invert=True)
        for r in (0, 1, 2.5):
            got = vol.expand_labels(r)
            assert got.is_cuda and got.dtype == torch.uint32 and np.array_equal(got.cpu().numpy(), expanded(grown, r)), r
        picked = nearest_twin(off, dens, labs, selected=[1, 0xFFFFFFF0], ignore_zero=True, invert=True)
        got = vol.expand_labels(2, labels=[1, 0xFFFFFFF0]).cpu().numpy()
        assert np.array_equal(got, expanded(picked, 2)) and set(np.unique(got)) == {0, 1, 0xFFFFFFF0}
        empty = vol.nearest(level=1.0, box=((0, 0, 0), (4, 4, 4)))                                        # misses the window
        assert empty.squared.numel() == 0 and empty.index.numel() == 0 and empty.targets == 0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        again = vol.nearest(invert=True, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(again.index.cpu().numpy(), grown["index"]) and np.array_equal(again.label.cpu().numpy(), grown["label"])
    finally:
        vol.world.scale = (1.0, 1.0, 1.0)
        vol.world.position = (0.0, 0.0, 0.0)


def test_refusals_enqueue_nothing():
    vol = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    arrays = [torch.full((64,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    sel = torch.tensor([1, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        p = N.NearestParams(lod=0, mode=N.COMPONENTS_LABELS, selected=sel.data_ptr(), selected_count=2)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return p

    def call(p=None, h=handle, null=(), cap=64):
        p = p or params()
        ptrs = [None if name in null else t.data_ptr() for name, t in zip(("d2", "index", "label"), arrays)]
        out = N.NearestOutputs(*ptrs, cap, None if "header" in null else header.data_ptr())
        return lib.svr_nearest(h, None if "params" in null else C.byref(p), None if "out" in null else C.byref(out), None)

    def untouched():
        torch.cuda.synchronize()
        return bool((header == -7).all()) and all(bool((t == -7).all()) for t in arrays)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("header",)), "null argument"),
        (dict(p=params(lod=-1)), "lod out of range"), (dict(p=params(lod=2)), "lod out of range"),
        (dict(p=params(mode=2)), "unknown mode"), (dict(p=params(mode=-1)), "unknown mode"),
        (dict(p=params(mode=N.COMPONENTS_LEVEL, level=float("nan"))), "level must not be NaN"),
        (dict(p=params(selected=None)), "NULL selected pointer"),
        (dict(p=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(null=("d2",)), "NULL d2"), (dict(null=("index",)), "NULL index"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        text = lib.svr_last_error().decode()
        assert text.startswith("svr_nearest: ") and msg in text, (msg, text)
    assert untouched()                                                                                     # nothing was enqueued
    # the two limits, on contexts of their own, whose memory no kernel touches: u8 rings without labels
    for ring, shapes, msg in (((1032, 1024, 1024), [None, (1025, 1024, 1024)], "svr_nearest: more than SVR_DISTANCE_MAX_VOXELS voxels"),
                              ((16392, 8, 8), [None, (16385, 1, 1)], "svr_nearest: an extent of more than SVR_DISTANCE_MAX_EXTENT voxels")):
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
                p = params(selected=None, selected_count=0) if shape is None else params(use_box=1, box_off=(0, 0, 0), box_shape=shape)
                assert call(p=p, h=other) == -1 and msg in lib.svr_last_error().decode(), (ring, shape)
                assert call(p=p, h=other, null=("d2", "index", "label"), cap=0) == -1                      # the count-only call too
        finally:
            N.check(lib.svr_destroy(other), "svr_destroy")
    assert untouched()
    # the control cases run: too small a capacity writes the header alone; NULL arrays with capacity 0 are the count-only call;
    # a NULL label is no refusal
    assert call(params(selected=None, selected_count=0)) == 0
    torch.cuda.synchronize()
    assert int(header[0]) > 4 and header[2:4].tolist() == [0, 0] and header[14:].tolist() == [0, 0] and all(bool((t == -7).all()) for t in arrays)
    assert call(null=("d2", "index", "label"), cap=0) == 0
    assert call(params(use_box=1, box_off=tuple(window_of(vol, 0)[0]), box_shape=(4, 4, 4)), null=("label",)) == 0
    torch.cuda.synchronize()
    assert int(header[2]) == 64 and bool((arrays[2] == -7).all()) and not bool((arrays[1] == -7).any())
