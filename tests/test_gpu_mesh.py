"""GPU: svr_mesh (include/svr.h) == the numpy restatement tests/mesh_twin.py, which reads the same window through
svr_read_region.  The header and the triangles are equal exactly, order included, in every case; the vertices are equal
bit for bit in SVR_MESH_LABELS and within 1e-4 voxel (the project's float tolerance against its restatements) in
SVR_MESH_LEVEL.  A ring of 72 x 16 x 40 voxels (LOD 1: 36 x 12 x 20) whose window wraps on all three axes, with objects
across each seam and one across the corner where the three seams meet; u8, u16 and float32 rings (NaN and infinities
planted); boxes that make rows of 16, 17 and 65 cells; word counts that need two and three levels of the scan; a volume
without label rings; capacities; reproducibility; ordering behind uploads; the Python surface; every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mesh_twin import area_volume, mesh_twin
from sub_volume_renderer_amd import Roi, _native as N, testing

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "sub_volume_renderer_amd", "csrc", "mesh_plan.h")).read()
SCAN_BLOCK = int(re.search(r"kMeshScanBlock = (\d+);", PLAN).group(1))
CELLS_PER_WORD = int(re.search(r"kMeshCellsPerWord = (\d+);", PLAN).group(1))
LEVEL = {"u8": 128.0, "u16": 128.0 * 251.0, "f32": 27.36}            # about half the voxels reach it
CENTRE = (84.0, 30.0, 36.0)                                          # world = data position (x, y, z)


def volumes(kind):
    """[(density, labels)] of LOD 0 (64 x 64 x 128, numpy order) and LOD 1 (every second voxel)."""
    z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(128), indexing="ij")
    rng = np.random.default_rng(7)
    d = ((3 * x + 5 * y + 2 * z + rng.integers(0, 90, x.shape)) % 256).astype(np.uint8)
    lab = np.array([0, 9, 10], np.uint32)[rng.integers(0, 3, x.shape)]          # a dense background of small objects
    lab[(x - 72) ** 2 + (y - 32) ** 2 + (z - 40) ** 2 <= 25] = 1                # across the corner where the three seams meet
    lab[(x >= 68) & (x < 76) & (y >= 27) & (y < 30) & (z >= 22) & (z < 27)] = 2             # across the x seam (72)
    lab[(x >= 56) & (x < 60) & (y >= 29) & (y < 35) & (z >= 44) & (z < 50)] = 3             # across the y seam (32)
    lab[(x >= 90) & (x < 95) & (y >= 27) & (y < 31) & (z >= 36) & (z < 44)] = 0xFFFFFFF0    # across the z seam (40)
    if kind == "u16":
        d = d.astype(np.uint16) * np.uint16(251)
    if kind == "f32":
        d = d.astype(f32) * f32(0.37) - f32(20.0)
        flat = d.reshape(-1)
        # inside the window of either LOD: even coordinates around the centre
        zz, yy, xx = (2 * rng.integers(c // 2 - 3, c // 2 + 3, 90) for c in (36, 30, 84))
        at = (zz * 64 + yy) * 128 + xx
        flat[at[:30]], flat[at[30:60]], flat[at[60:]] = np.nan, np.inf, -np.inf
    pairs = [(d, lab), (d[::2, ::2, ::2].copy(), lab[::2, ::2, ::2].copy())]
    if kind == "nolabels":
        pairs = [(p, None) for p, _ in pairs]
    return pairs


def spec_of(kind):
    data = {"twin_all": "u8", "twin_off": "u8", "nolabels": "u8"}.get(kind, kind)
    spec = testing.synthetic_spec(64, 32, 32, pairs=volumes("nolabels" if kind == "nolabels" else data),
                                  chunk_shapes=[(8, 8, 8), (4, 4, 4)], ring_shapes=[(5, 2, 9), (5, 3, 9)])
    spec.centers = [(CENTRE, None)]
    if kind == "twin_all":
        spec.blocked_twin = "all"
    if kind == "twin_off":
        spec.blocked_twin = False
    return spec


_SCENES = {}


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


_WINDOWS = {}


def window_of(vol, lod, fresh=False):
    """(offset (x, y, z), density f32 [z][y][x], labels u32 or None) of the LOD's window, through svr_read_region of the
    whole ring and the window's ring slots; read once per volume and LOD unless ``fresh``."""
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


def c_mesh(vol, lod, *, box=None, labels=None, level=None, vcap=None, tcap=None, fill=-7):
    """One svr_mesh call through the C ABI into pattern-filled arrays of the given capacities (None: the count-only call
    with NULL arrays) -> (header as 8 Python ints, vertices f32 [vcap, 3], triangles i32 [tcap, 3])."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    mp = N.MeshParams(lod=lod)
    if box is not None:
        mp.use_box = 1
        mp.box_off[:], mp.box_shape[:] = box
    sel = None
    if labels is not None:
        mp.mode = N.MESH_LABELS
        sel = torch.from_numpy(np.unique(np.asarray(labels, np.uint32)).view(np.int32)).to(dev)
        mp.selected, mp.selected_count = sel.data_ptr(), sel.numel()
    else:
        mp.mode, mp.level = N.MESH_LEVEL, level
    header = torch.full((8,), fill, dtype=torch.int64, device=dev)
    vertices = None if vcap is None else torch.full((vcap, 3), float(fill), dtype=torch.float32, device=dev)
    triangles = None if tcap is None else torch.full((tcap, 3), fill, dtype=torch.int32, device=dev)
    mo = N.MeshOutputs(None if vertices is None else vertices.data_ptr(), None if triangles is None else triangles.data_ptr(),
                       header.data_ptr(), vcap or 0, tcap or 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().svr_mesh(handle, C.byref(mp), C.byref(mo), C.c_void_p(stream)), "svr_mesh")
    torch.cuda.synchronize()
    return ([int(v) for v in header.cpu().numpy()], None if vertices is None else vertices.cpu().numpy(),
            None if triangles is None else triangles.cpu().numpy())


def hold(vol, lod, what, *, box=None, labels=None, level=None, window=None):
    """Count, then emit into exact capacities, and hold both to the twin.  -> the twin's result."""
    off, shape, ring, dens, labs = window or window_of(vol, lod)
    twin = mesh_twin(off, dens, labs, box=box, selected=labels, level=level)
    V, T = twin["header"][0], twin["header"][1]
    head, _, _ = c_mesh(vol, lod, box=box, labels=labels, level=level)
    assert head == twin["header"][:2] + [0, 0] + twin["header"][4:], (what, "count", head, twin["header"])
    head, v, t = c_mesh(vol, lod, box=box, labels=labels, level=level, vcap=V, tcap=T)
    assert head == twin["header"], (what, head, twin["header"])
    assert np.array_equal(t, twin["triangles"]), (what, "triangles")
    if labels is not None:
        assert np.array_equal(v.view(np.uint32), twin["vertices"].view(np.uint32)), (what, "vertices", float(np.abs(v - twin["vertices"]).max()))
    elif V:
        assert float(np.abs(v - twin["vertices"]).max()) <= 1e-4, (what, "vertices", float(np.abs(v - twin["vertices"]).max()))
    return twin


def boxes_of(off, shape):
    """(name, box) in the LOD's logical voxels, anchored to the window."""
    ox, oy, oz = off
    return [
        ("window", None),
        ("partly outside", ((ox - 5, oy + 2, oz + shape[2] - 6), (20, shape[1] + 9, 30))),
        ("inner, odd", ((ox + 3, oy + 1, oz + 2), (29, 7, 5))),
        ("one voxel", ((ox + 7, oy + 3, oz + 9), (1, 1, 1))),
        ("misses", ((ox + shape[0] + 4, oy, oz), (4, 4, 4))),
        ("empty shape", ((ox + 4, oy + 2, oz + 2), (0, 5, 5))),
    ]


def test_the_window_wraps_on_all_three_axes():
    for kind in ("u8", "f32"):
        vol = scene_of(kind)
        for lod in (0, 1):
            off, shape, ring, dens, labs = window_of(vol, lod)
            assert ring == ((40, 16, 72) if lod == 0 else (20, 12, 36))
            for a in range(3):
                assert off[a] % ring[2 - a] + shape[a] > ring[2 - a], (lod, a, off, shape)
            assert min(shape) >= 8 and shape[0] >= (64 if lod == 0 else 32)
    off, shape, ring, dens, labs = window_of(scene_of("u8"), 0)
    for label in (1, 2, 3, 0xFFFFFFF0):                                # every seam object lies in the window, on both sides of its seam
        z, y, x = np.nonzero(labs == label)
        assert z.size > 30
    x = np.nonzero(labs == 2)[2] + off[0]
    assert x.min() < 72 <= x.max()
    dens = window_of(scene_of("f32"), 0)[3]
    assert np.isnan(dens).any() and np.isposinf(dens).any() and np.isneginf(dens).any()


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("lod", [0, 1])
def test_labels_and_level(kind, lod):
    vol = scene_of(kind)
    off, shape, ring, dens, labs = window_of(vol, lod)
    for name, box in boxes_of(off, shape):
        twin = hold(vol, lod, (kind, lod, name, "labels"), box=box, labels=[1, 2, 3, 0xFFFFFFF0, 77])
        if name in ("misses", "empty shape"):
            assert twin["header"][:4] == [0, 0, 0, 0] and twin["header"][7] == 0
        elif name == "window":                                         # LOD 1 holds an eighth of the seam objects' voxels
            assert twin["header"][0] > (300 if lod == 0 else 60) and twin["header"][7] > (300 if lod == 0 else 40)
        twin = hold(vol, lod, (kind, lod, name, "level"), box=box, level=LEVEL[kind])
        if name == "window":
            share = twin["header"][7] / float(np.prod(shape))
            assert 0.3 < share < 0.7 and twin["header"][0] > (2000 if lod == 0 else 300), share
    hold(vol, lod, (kind, lod, "dense labels"), labels=[9])           # a third of all voxels: every kind of cell
    if kind == "f32":
        for level in (-np.inf, np.inf, 3e38, -25.0):
            hold(vol, lod, (kind, lod, "level", level), level=float(level))


def test_rows_of_16_17_and_65_cells_and_the_scan_levels():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    assert shape[0] >= 64
    for cells in (15, 16, 17, 33, 64, 65):
        for start in (0, 1, 7):                                        # the row's first voxel in every alignment class that matters
            box = ((off[0] + start, off[1] + 3, off[2] + 20), (cells - 1, 9, 25))
            if start + cells - 1 > shape[0]:
                continue
            hold(vol, 0, ("row", cells, start), box=box, labels=[9, 1])
            hold(vol, 0, ("row", cells, start, "level"), box=box, level=LEVEL["u8"])
    # one block of the scan holds the words of a small box; the whole window needs the block sums above it
    words = lambda n: -(-(n[0] + 1) // CELLS_PER_WORD) * (n[1] + 1) * (n[2] + 1)
    assert SCAN_BLOCK < words(shape) <= SCAN_BLOCK ** 2
    assert words((15, 15, 15)) == SCAN_BLOCK                           # exactly one block ...
    hold(vol, 0, "one scan block", box=((off[0] + 2, off[1], off[2] + 1), (15, 15, 15)), labels=[9])
    hold(vol, 0, "one word more", box=((off[0] + 2, off[1], off[2] + 1), (16, 15, 15)), labels=[9])      # ... and twice as many words


def test_three_levels_of_the_scan():
    """A window of more than kMeshScanBlock^2 words: the block sums have block sums of their own."""
    rng = np.random.default_rng(11)
    n = 112
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    lab = ((x // 5 + y // 3 + z // 4) % 3).astype(np.uint32)
    lab[rng.random(lab.shape) < 0.02] = 1
    d = ((x + y + z) % 256).astype(np.uint8)
    spec = testing.synthetic_spec(n, 32, 32, pairs=[(d, lab)], chunk_shapes=[(8, 8, 8)], ring_shapes=[(13, 13, 13)])
    spec.centers = [((60.0, 58.0, 62.0), None)]
    vol = testing.build(spec).volume
    try:
        window = window_of(vol, 0)
        off, shape = window[0], window[1]
        words = -(-(shape[0] + 1) // CELLS_PER_WORD) * (shape[1] + 1) * (shape[2] + 1)
        assert words > SCAN_BLOCK ** 2, (shape, words)
        assert any(off[a] % 104 + shape[a] > 104 for a in range(3))
        twin = hold(vol, 0, "three levels", labels=[1], window=window)
        assert twin["header"][0] > 50000
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_without_label_rings():
    vol = scene_of("nolabels")
    assert not vol._rings.labels
    for lod in (0, 1):
        off, shape, ring, dens, labs = window_of(vol, lod)
        assert labs is None
        twin = hold(vol, lod, "no labels, {0}", labels=[0, 5])          # the solid box of the window
        a, b, c = shape
        assert twin["header"][7] == a * b * c and twin["header"][1] == 4 * (a * b + b * c + a * c)
        assert hold(vol, lod, "no labels, {5}", labels=[5])["header"][:4] == [0, 0, 0, 0]
        hold(vol, lod, "no labels, level", level=LEVEL["u8"])


def test_capacities():
    vol = scene_of("u8")
    off, shape, ring, dens, labs = window_of(vol, 0)
    for mode in (dict(labels=[1, 2, 3]), dict(level=LEVEL["u8"])):
        twin = mesh_twin(off, dens, labs, selected=mode.get("labels"), level=mode.get("level"))
        V, T = twin["header"][:2]
        assert V > 100 and T > 100
        for vcap, tcap in ((V - 1, T), (V, T - 1), (V - 1, T + 5), (1, 1)):
            head, v, t = c_mesh(vol, 0, vcap=vcap, tcap=tcap, **mode)
            assert head == [V, T, 0, 0] + twin["header"][4:], (vcap, tcap, head)
            assert (v == -7.0).all() and (t == -7).all(), (vcap, tcap)             # neither array was touched
        for vcap, tcap in ((V, T), (V + 3, T + 2)):
            head, v, t = c_mesh(vol, 0, vcap=vcap, tcap=tcap, **mode)
            assert head == twin["header"]
            assert np.array_equal(t[:T], twin["triangles"]) and (t[T:] == -7).all() and (v[V:] == -7.0).all()
            assert np.abs(v[:V] - twin["vertices"]).max() <= (0.0 if "labels" in mode else 1e-4)
        # a count-only call with one array given: nothing is written either
        head, v, t = c_mesh(vol, 0, vcap=V, tcap=None, **mode)
        assert head[:4] == [V, T, 0, 0] and (v == -7.0).all()


def test_two_calls_give_identical_bytes_with_or_without_the_micro_block_copy():
    with_copy, without = scene_of("twin_all"), scene_of("twin_off")
    assert any(with_copy._rings.blocked_twin) and not any(without._rings.blocked_twin)
    for lod in (0, 1):
        for mode in (dict(labels=[9, 1]), dict(level=LEVEL["u8"])):
            twin = hold(with_copy, lod, ("copy", lod), **mode)
            V, T = twin["header"][:2]
            runs = [c_mesh(vol, lod, vcap=V, tcap=T, **mode) for vol in (with_copy, with_copy, without, without)]
            for head, v, t in runs[1:]:
                assert head == runs[0][0] and v.tobytes() == runs[0][1].tobytes() and t.tobytes() == runs[0][2].tobytes()


def test_a_call_right_after_an_upload_sees_it():
    spec = spec_of("u8")
    vol = testing.build(spec).volume
    try:
        lib, handle = N.lib(), vol.prepare()
        off, shape, ring, dens, labs = window_of(vol, 0)
        buf = vol.wrapping_buffers[0]
        rng = np.random.default_rng(2)
        for step in range(3):
            # a block of new values and labels into ring slots of the window, published, and the mesh right behind it
            block_d = rng.integers(0, 256, (16, 8, 24)).astype(np.uint8)
            block_l = rng.integers(0, 3, (16, 8, 24)).astype(np.uint32)
            buf._upload(Roi((8 * step, 4, 16 * step), (16, 8, 24)), block_d, block_l)
            N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
            got = [c_mesh(vol, 0, labels=[1]), c_mesh(vol, 0, level=100.0)]
            window = window_of(vol, 0, fresh=True)
            assert got[0][0][:2] == mesh_twin(window[0], window[3], window[4], selected=[1])["header"][:2], step
            assert got[1][0][:2] == mesh_twin(window[0], window[3], window[4], level=100.0)["header"][:2], step
            hold(vol, 0, ("after upload", step), labels=[1, 2], window=window)
        N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
        N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
        head, _, _ = c_mesh(vol, 0, level=1.0)
        assert head[:4] == [0, 0, 0, 0] and head[7] == 0
        head, _, _ = c_mesh(vol, 0, labels=[0])
        a, b, c = shape
        assert head[7] == a * b * c and head[1] == 4 * (a * b + b * c + a * c)
    finally:
        _WINDOWS.pop((id(vol), 0), None)
        vol.close()


def test_python_surface(tmp_path):
    vol = scene_of("u8")
    vol.world.scale = (1.5, 0.5, 2.0)
    vol.world.position = (3.0, -2.0, 7.0)
    try:
        for lod, kw in ((0, dict(labels=[3, 1, 3, 2])), (1, dict(level=LEVEL["u8"])), (0, dict(level=LEVEL["u8"], box=((20, 26, 50), (44, 36, 90))))):
            off, shape, ring, dens, labs = window_of(vol, lod)
            box = None
            if "box" in kw:
                b, e = kw["box"]
                box = (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))            # LOD 0: scale 1
            twin = mesh_twin(off, dens, labs, box=box, selected=kw.get("labels"), level=kw.get("level"))
            m = vol.mesh(lod=lod, **kw)
            assert m.vertices.is_cuda and m.vertices.dtype == torch.float32 and m.triangles.dtype == torch.int32
            assert tuple(m.vertices.shape) == (twin["header"][0], 3) and tuple(m.triangles.shape) == (twin["header"][1], 3)
            assert np.array_equal(m.triangles.cpu().numpy(), twin["triangles"])
            assert np.abs(m.vertices.cpu().numpy() - twin["vertices"]).max() <= (0.0 if "labels" in kw else 1e-4)
            assert list(m.offset) == off and m.inside_voxels == twin["header"][7] and m.lod == lod and len(m) == twin["header"][1]
            # f64 numpy on the twin's mesh: data coordinates (c + 0.5) / scale - 0.5, then the world transform
            scale = np.array(vol.wrapping_buffers[lod].scale_factor[::-1], np.float64)
            data = (m.vertices.cpu().numpy().astype(np.float64) + np.array(off, np.float64) + 0.5) / scale - 0.5
            world = data * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0])
            assert np.abs(m.data_vertices().cpu().numpy() - data).max() <= 1e-12
            assert np.abs(m.world_vertices().cpu().numpy() - world).max() <= 1e-11
            area, volume = area_volume(world, twin["triangles"])
            assert volume > 0 and abs(m.area() - area) <= 1e-9 * area and abs(m.enclosed_volume() - volume) <= 1e-9 * volume
            path = tmp_path / f"mesh{lod}.obj"
            m.write_obj(path)
            lines = open(path).read().split("\n")
            vs = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")])
            fs = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("f ")])
            assert np.array_equal(vs, m.world_vertices().cpu().numpy()) and np.array_equal(fs - 1, twin["triangles"])
        empty = vol.mesh(labels=[123456])
        assert len(empty) == 0 and tuple(empty.vertices.shape) == (0, 3) and empty.inside_voxels == 0 and empty.area() == 0.0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        m = vol.mesh(labels=[1], stream=side.cuda_stream)
        side.synchronize()
        off, shape, ring, dens, labs = window_of(vol, 0)
        assert np.array_equal(m.triangles.cpu().numpy(), mesh_twin(off, dens, labs, selected=[1])["triangles"])
    finally:
        vol.world.scale = (1.0, 1.0, 1.0)
        vol.world.position = (0.0, 0.0, 0.0)


def test_refusals_enqueue_nothing():
    vol = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    header = torch.full((8,), -7, dtype=torch.int64, device=dev)
    vertices = torch.full((64, 3), -7.0, dtype=torch.float32, device=dev)
    triangles = torch.full((64, 3), -7, dtype=torch.int32, device=dev)
    sel = torch.tensor([1, 5], dtype=torch.int32, device=dev)

    def params(**kw):
        mp = N.MeshParams(lod=0, mode=N.MESH_LABELS, selected=sel.data_ptr(), selected_count=2)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(mp, k)[:] = v
            else:
                setattr(mp, k, v)
        return mp

    def call(mp=None, h=handle, null=(), vcap=64, tcap=64):
        mp = mp or params()
        mo = N.MeshOutputs(None if "vertices" in null else vertices.data_ptr(), None if "triangles" in null else triangles.data_ptr(),
                           None if "header" in null else header.data_ptr(), vcap, tcap)
        return lib.svr_mesh(h, None if "params" in null else C.byref(mp), None if "out" in null else C.byref(mo), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("header",)), "null argument"),
        (dict(mp=params(lod=-1)), "lod out of range"), (dict(mp=params(lod=2)), "lod out of range"),
        (dict(mp=params(mode=2)), "unknown mode"), (dict(mp=params(mode=-1)), "unknown mode"),
        (dict(mp=params(selected_count=0)), "at least one selected id"), (dict(mp=params(selected=None)), "at least one selected id"),
        (dict(mp=params(mode=N.MESH_LEVEL, level=float("nan"))), "level must not be NaN"),
        (dict(mp=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(null=("vertices",)), "NULL vertices"), (dict(null=("triangles",)), "NULL triangles"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((vertices == -7.0).all()) and bool((triangles == -7).all())       # nothing was enqueued
    # the control cases run: too small a capacity writes the header alone; NULL arrays with capacity 0 are the count-only call
    assert call() == 0
    torch.cuda.synchronize()
    assert int(header[0]) > 64 and header[2:4].tolist() == [0, 0] and bool((vertices == -7.0).all()) and bool((triangles == -7).all())
    assert call(null=("vertices", "triangles"), vcap=0, tcap=0) == 0
    assert call(params(mode=N.MESH_LEVEL, level=float("inf"), selected=None, selected_count=0)) == 0
    assert call(params(box_shape=(4, -1, 4))) == 0                      # use_box == 0 makes the box irrelevant
    torch.cuda.synchronize()
