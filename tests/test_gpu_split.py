"""GPU: svr_split (include/svr.h) == the numpy restatement tests/split_twin.py: the header, the dense numbers and every
field of every record are equal exactly, in every case.  Through the C ABI on height fields made here (random heights
with many ties, the squared distances of two overlapping balls, an all-FAR plateau) in boxes from one voxel to one whose
scan has a second level, and one of isolated voxels whose scan has a third; capacities; reproducibility; two streams;
every refusal.  Through SubVolume.split on a two-LOD scene whose rings are 21 voxels wide along x and whose windows wrap them."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from distance_twin import FAR, distance_twin, squared_edt
from split_twin import RECORD, count_only, split_twin
from sub_volume_renderer_amd import Roi, _native as N, testing

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A
MERGES = (0, 1, 9, 1 << 29)
BOXES = [(1, 1, 1), (5, 1, 1), (1, 1, 7), (63, 5, 3), (65, 9, 4), (67, 33, 31)]        # (n_x, n_y, n_z)
LEVEL = 128.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_BLOCK = int(re.search(r"kBoxScanBlock = (\d+);", open(os.path.join(ROOT, "sub_volume_renderer_amd", "csrc", "box_scan.h")).read()).group(1))

_SCENE = {}


def volumes():
    """[(density, labels)] of LOD 0 (48 x 48 x 84, numpy order) and LOD 1 (every second voxel): pairs and chains of
    overlapping balls, bright on a dim noise, each chain one label."""
    z, y, x = np.meshgrid(np.arange(48), np.arange(48), np.arange(84), indexing="ij")
    rng = np.random.default_rng(21)
    d = rng.integers(0, 100, x.shape).astype(np.uint8)
    lab = np.zeros(x.shape, np.uint32)
    chains = [(1, [(38, 26, 28, 5), (45, 27, 28, 5)]), (2, [(40, 20, 19, 3), (44, 20, 19, 3)]), (3, [(37, 34, 34, 4), (43, 35, 34, 4)]),
              (0xFFFFFFF0, [(47, 33, 22, 3)])]
    for label, balls in chains:
        for cx, cy, cz, r in balls:
            m = (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r
            d[m] = 200
            lab[m] = label
    return [(d, lab), (d[::2, ::2, ::2].copy(), lab[::2, ::2, ::2].copy())]


def scene():
    if "vol" not in _SCENE:
        spec = testing.synthetic_spec(64, 32, 32, pairs=volumes(), chunk_shapes=[(8, 8, 3), (4, 4, 3)], ring_shapes=[(4, 4, 7), (4, 4, 7)])
        spec.centers = [((42.0, 28.0, 28.0), None)]
        _SCENE["vol"] = testing.build(spec).volume
    return _SCENE["vol"]


@pytest.fixture(scope="module", autouse=True)
def _close_scene():
    yield
    if "vol" in _SCENE:
        _SCENE.pop("vol").close()
    _SCENE.clear()


def window_of(vol, lod):
    """(offset (x, y, z), shape, ring (numpy order), density f32 [z][y][x], labels u32) of the LOD's window, through
    svr_read_region of the whole ring and the window's ring slots; read once per LOD."""
    if ("window", lod) not in _SCENE:
        st = N.LodState()
        N.check(N.lib().svr_get_lod_state(vol.prepare(), lod, C.byref(st)), "svr_get_lod_state")
        off, shape = [int(v) for v in st.offset], [int(v) for v in st.shape]
        buf = vol.wrapping_buffers[lod]
        ring = tuple(int(v) for v in buf.shape_in_pixels)
        dens, labs = buf.read_ring(Roi((0, 0, 0), ring))
        idx = np.ix_(*[(off[a] + np.arange(shape[a])) % ring[2 - a] for a in (2, 1, 0)])
        _SCENE[("window", lod)] = (off, shape, ring, dens[idx], labs[idx])
    return _SCENE[("window", lod)]


def fields(box):
    """[(name, height int32 [n_z][n_y][n_x])] of a box (n_x, n_y, n_z)."""
    nx, ny, nz = box
    rng = np.random.default_rng(nx * 10007 + ny * 101 + nz)
    z, y, x = np.indices((nz, ny, nx))
    r = max(min(nx, ny, nz) // 2, max(nx, ny, nz) // 4, 1)
    axis = int(np.argmax((nz, ny, nx)))
    centres = []
    for t in (0.5 - 0.19, 0.5 + 0.19):                                 # 0.38 of the long axis apart: they overlap where r is its quarter
        c = [nz // 2, ny // 2, nx // 2]
        c[axis] = int((nz, ny, nx)[axis] * t)
        centres.append(c)
    inside = np.zeros((nz, ny, nx), bool)
    for c in centres:
        inside |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
    return [("random", (rng.integers(0, 4, (nz, ny, nx)) * (rng.random((nz, ny, nx)) < 0.75)).astype(np.int32)),
            ("balls", squared_edt(~inside, border=True)),
            ("far", np.full((nz, ny, nx), FAR, np.int32))]


def c_split(height, connectivity, merge_squared, ids_cap=None, rec_cap=None, stream=None, sync=True):
    """One svr_split call through the C ABI into pattern-filled arrays of the given capacities (None: NULL and 0) ->
    (header as 16 Python ints, ids u32 [ids_cap] or None, records RECORD [rec_cap] or None); with ``sync=False`` the
    device tensors (header, ids, records, height), for the caller to read once the device is idle."""
    vol = scene()
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    nz, ny, nx = height.shape
    h = torch.from_numpy(np.ascontiguousarray(height, np.int32)).to(dev)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    ids = None if ids_cap is None else torch.from_numpy(np.full(ids_cap, FILL, np.uint32).view(np.int32)).to(dev)
    records = None if rec_cap is None else torch.from_numpy(np.full((rec_cap, 20), FILL, np.uint32).view(np.int32)).to(dev)
    sp = N.SplitParams(height=h.data_ptr(), connectivity=connectivity, merge_squared=merge_squared)
    sp.n[:] = (nx, ny, nz)
    so = N.SplitOutputs(None if ids is None else ids.data_ptr(), ids_cap or 0, None if records is None else records.data_ptr(), rec_cap or 0,
                        header.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    N.check(N.lib().svr_split(handle, C.byref(sp), C.byref(so), C.c_void_p(s)), "svr_split")
    if not sync:
        return header, ids, records, h
    torch.cuda.synchronize()
    return read_back(header, ids, records)


def read_back(header, ids, records):
    return ([int(v) for v in header.cpu().numpy().view(np.uint64)], None if ids is None else ids.cpu().numpy().view(np.uint32),
            None if records is None else records.cpu().numpy().view(np.uint32).reshape(-1).view(RECORD))


def same_records(got, want, what):
    assert len(got) == len(want), what
    for name in RECORD.names:
        assert np.array_equal(got[name], want[name]), (what, name)


def hold(height, connectivity, H, what, twin=None):
    """Count, then emit into capacities one beyond exact, and hold both to the twin.  -> the twin's result."""
    twin = twin or split_twin(height, connectivity, H)
    want = twin["header"]
    head, _, _ = c_split(height, connectivity, H)
    assert head == count_only(want), (what, "count", head, want)
    head, ids, records = c_split(height, connectivity, H, ids_cap=want[2] + 1, rec_cap=want[0] + 1)
    assert head == want, (what, head, want)
    assert np.array_equal(ids[:want[2]], twin["ids"].reshape(-1)), (what, "ids", int((ids[:want[2]] != twin["ids"].reshape(-1)).sum()))
    same_records(records[:want[0]], twin["records"], what)
    assert (ids[want[2]:] == FILL).all() and (records[want[0]:].view(np.uint32) == FILL).all(), (what, "beyond the end")
    return twin


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "x".join(str(v) for v in b))
def test_through_the_c_abi(box):
    seen = set()
    for name, height in fields(box):
        for connectivity in (6, 26):
            for H in MERGES:
                twin = hold(height, connectivity, H, (box, name, connectivity, H))
                seen.add(twin["header"][0])
                if name == "far":
                    assert twin["header"][:2] == [1, height.size] and twin["records"]["peak"].tolist() == [FAR]
                if name == "balls" and min(box) > 1:
                    assert twin["header"][1] > 0 and twin["header"][0] >= 1
    if box == (67, 33, 31):
        assert -(-67 * 33 * 31 // 256) > 256 and max(seen) > 256         # a scan of two levels, and regions beyond its first block


def test_three_levels_of_the_scan():
    """More than SCAN_BLOCK^2 blocks of voxels: the block sums of the u32 scan (csrc/box_scan.h), which svr_components runs
    in the same instantiation, have block sums of their own, level 1 fills more than one block and the top holds two
    entries.  Positive heights on a thinned checkerboard: no two positive voxels are 6-neighbours, so every one is its own
    summit and its own region, and its number is the count of positive voxels up to and including it.  The thinning makes
    the counts per block differ, so that a wrong prefix at any level shows."""
    nx, ny, nz = 260, 256, 256
    voxels = nx * ny * nz
    count = [-(-voxels // SCAN_BLOCK)]
    while count[-1] > SCAN_BLOCK:
        count.append(-(-count[-1] // SCAN_BLOCK))
    assert voxels == 17039360 and count == [66560, 260, 2]
    rng = np.random.default_rng(29)
    z, y, x = np.ogrid[:nz, :ny, :nx]
    keep = ((x + y + z) % 2 == 0) & (rng.random((nz, ny, nx)) < 2.0 / 3.0)
    height = np.where(keep, rng.integers(1, 1000, (nz, ny, nx)), 0).astype(np.int32)
    header, ids, _, h = c_split(height, 6, 0, ids_cap=voxels, sync=False)
    torch.cuda.synchronize()
    positive = (h.reshape(-1) > 0).to(torch.int32)
    want = torch.cumsum(positive, 0, dtype=torch.int32) * positive
    n = int(positive.sum())
    assert n == int(keep.sum()) and voxels // 4 < n < voxels // 2
    head = [int(v) for v in header.cpu().numpy().view(np.uint64)]
    assert head[0] == n and head[1] == n and head[2] == voxels, head
    assert torch.equal(ids, want)
    del header, ids, h, want, positive
    torch.cuda.empty_cache()
    head, _, _ = c_split(height, 6, 0)
    assert head[0] == n, head
    torch.cuda.empty_cache()


def test_capacities():
    height = fields((65, 9, 4))[0][1]
    twin = split_twin(height, 26, 0)
    want, n, count = twin["header"], twin["header"][2], twin["header"][0]
    assert count > 3
    flat = twin["ids"].reshape(-1)
    # one capacity one short: that array is untouched bit for bit, the other is written
    head, ids, records = c_split(height, 26, 0, ids_cap=n - 1, rec_cap=count)
    assert head == want[:2] + [0, count] + want[4:] and (ids == FILL).all()
    same_records(records, twin["records"], "ids one short")
    head, ids, records = c_split(height, 26, 0, ids_cap=n, rec_cap=count - 1)
    assert head == want[:3] + [0] + want[4:] and (records.view(np.uint32) == FILL).all() and np.array_equal(ids, flat)
    # records without ids, ids without records
    head, ids, records = c_split(height, 26, 0, rec_cap=count)
    assert head == want[:2] + [0, count] + want[4:] and ids is None
    same_records(records, twin["records"], "records alone")
    head, ids, records = c_split(height, 26, 0, ids_cap=n)
    assert head == want[:3] + [0] + want[4:] and records is None and np.array_equal(ids, flat)
    # both short: the count-only header
    head, ids, records = c_split(height, 26, 0, ids_cap=n - 1, rec_cap=count - 1)
    assert head == count_only(want) and (ids == FILL).all() and (records.view(np.uint32) == FILL).all()


def test_two_calls_and_two_streams_give_identical_bytes():
    vol = scene()
    dev = torch.device("cuda", vol._rings.device)
    name, height = fields((67, 33, 31))[0]
    twin = split_twin(height, 26, 1)
    n, count = twin["header"][2], twin["header"][0]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    runs = [c_split(height, 26, 1, ids_cap=n, rec_cap=count) for _ in range(2)]
    runs += [c_split(height, 26, 1, ids_cap=n, rec_cap=count, stream=s.cuda_stream) for s in streams]
    for head, ids, records in runs:
        assert head == twin["header"] and ids.tobytes() == twin["ids"].tobytes() and records.tobytes() == twin["records"].tobytes()
    # two calls in flight on two streams at once, on different inputs: the second is ordered behind the first in the shared scratch
    other = fields((65, 9, 4))[1][1]
    cases = [(height, 26, 1, twin), (other, 6, 9, split_twin(other, 6, 9))]
    outs = []
    torch.cuda.synchronize()
    for s, (h, connectivity, H, want) in zip(streams, cases):
        outs.append(c_split(h, connectivity, H, ids_cap=want["header"][2], rec_cap=max(want["header"][0], 1), stream=s.cuda_stream, sync=False))
    torch.cuda.synchronize()
    for (header, ids, records, _), (h, connectivity, H, want) in zip(outs, cases):
        head, ids, records = read_back(header, ids, records)
        assert head == want["header"] and np.array_equal(ids, want["ids"].reshape(-1))
        same_records(records[:want["header"][0]], want["records"], "in flight together")


def test_refusals_enqueue_nothing():
    vol = scene()
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    header = torch.full((16,), -7, dtype=torch.int64, device=dev)
    ids = torch.full((64,), -7, dtype=torch.int32, device=dev)
    records = torch.full((4, 20), -7, dtype=torch.int32, device=dev)
    height = torch.ones((64,), dtype=torch.int32, device=dev)

    def params(n=(4, 4, 4), connectivity=26, merge_squared=1, null_height=False):
        sp = N.SplitParams(height=None if null_height else height.data_ptr(), connectivity=connectivity, merge_squared=merge_squared)
        sp.n[:] = n
        return sp

    def call(sp=None, h=handle, null=(), ids_cap=64, rec_cap=4):
        sp = sp or params()
        so = N.SplitOutputs(None if "ids" in null else ids.data_ptr(), ids_cap, None if "records" in null else records.data_ptr(), rec_cap,
                            None if "header" in null else header.data_ptr())
        return lib.svr_split(h, None if "params" in null else C.byref(sp), None if "out" in null else C.byref(so), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(null=("header",)), "null argument"), (dict(sp=params(null_height=True)), "null argument"),
        (dict(sp=params(connectivity=18)), "connectivity must be 6 or 26"), (dict(sp=params(connectivity=0)), "connectivity must be 6 or 26"),
        (dict(sp=params(merge_squared=(1 << 29) + 1)), "merge_squared above SVR_SPLIT_MAX_MERGE"),
        (dict(sp=params(merge_squared=0xFFFFFFFF)), "merge_squared above SVR_SPLIT_MAX_MERGE"),
        (dict(sp=params(n=(0, 4, 4))), "every extent must be > 0"), (dict(sp=params(n=(4, -1, 4))), "every extent must be > 0"),
        (dict(sp=params(n=(4, 4, -2147483648))), "every extent must be > 0"),
        (dict(sp=params(n=(1024, 1024, 1025))), "more than SVR_SPLIT_MAX_VOXELS voxels"),
        (dict(sp=params(n=(2147483647, 2147483647, 2147483647))), "more than SVR_SPLIT_MAX_VOXELS voxels"),
        (dict(null=("ids",)), "NULL ids with a non-zero ids_capacity"), (dict(null=("records",)), "NULL records with a non-zero record_capacity"),
    ]
    for kw, text in cases:
        assert call(**kw) == -1, kw
        message = lib.svr_last_error().decode()
        assert message.startswith("svr_split: ") and text in message, (kw, message)
    torch.cuda.synchronize()
    assert bool((header == -7).all()) and bool((ids == -7).all()) and bool((records == -7).all())
    # and the same arguments, valid, are taken: NULL arrays with capacities of 0
    assert call(null=("ids", "records"), ids_cap=0, rec_cap=0) == 0
    torch.cuda.synchronize()
    assert [int(v) for v in header.cpu().numpy()][:5] == [1, 64, 0, 0, 1] and bool((ids == -7).all())


def test_python_surface():
    vol = scene()
    vol.world.scale = (1.5, 0.5, 2.0)
    vol.world.position = (3.0, -2.0, 7.0)
    try:
        for lod in (0, 1):
            off, shape, ring, dens, labs = window_of(vol, lod)
            assert ring[2] == 21 and off[0] % 21 + shape[0] > 21, (lod, off, shape, ring)          # odd along x, and the window wraps it
        counts = []
        for lod, kw, mode, merge, connectivity in (
                (0, dict(level=LEVEL), dict(level=LEVEL), 1.0, 26),
                (0, dict(level=LEVEL), dict(level=LEVEL), 0, 6),
                (1, dict(level=LEVEL), dict(level=LEVEL), 1.5, 26),
                (0, dict(labels=[1, 3, 0xFFFFFFF0]), dict(selected=[1, 3, 0xFFFFFFF0], ignore_zero=True), 1.0, 26),
                (1, dict(labels=[2, 1]), dict(selected=[1, 2], ignore_zero=True), 2.0, 6),
                (0, dict(level=LEVEL, box="seam"), dict(level=LEVEL), 1.0, 26)):
            off, shape, ring, dens, labs = window_of(vol, lod)
            if kw.get("box") == "seam":                                 # a box of LOD 0 across the ring's x seam, cut by the window on y and z
                seam = off[0] + 21 - off[0] % 21
                b, e = (off[2] + 2, off[1] - 3, seam - 5), (off[2] + 20, off[1] + 17, seam + 4)     # numpy order, finest voxels = LOD 0 voxels
                kw = dict(kw, box=(b, e))
                mode = dict(mode, box=(b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1]))))
            field = distance_twin(off, dens, labs, border=True, **mode)
            H = int(np.floor(merge * merge))
            twin = split_twin(field["d2"], connectivity, H)
            got = vol.split(lod=lod, merge=merge, connectivity=connectivity, **kw)
            head, rec = twin["header"], twin["records"]
            what = (lod, kw, merge, connectivity)
            assert head[4] >= head[0] >= 1, what
            counts.append((head[0], head[4]))
            assert got.ids.is_cuda and got.ids.dtype == torch.int32 and tuple(got.ids.shape) == twin["ids"].shape
            assert np.array_equal(got.ids.cpu().numpy().view(np.uint32), twin["ids"]), what
            assert (got.count, got.inside_voxels, got.basins, got.lod, got.merge_squared, got.connectivity) == (head[0], head[1], head[4], lod, H, connectivity)
            begin = np.array(field["header"][7:10][::-1], np.int64)
            assert tuple(got.begin) == tuple(begin) and tuple(got.offset) == tuple(off[::-1])
            assert np.array_equal(got.voxels.cpu().numpy(), rec["voxels"].astype(np.int64))
            assert np.array_equal(got.region_basins.cpu().numpy(), rec["basins"].astype(np.int64))
            assert np.array_equal(got.peak_squared.cpu().numpy(), rec["peak"].astype(np.int64))
            assert np.array_equal(got.top.cpu().numpy(), begin + rec["top"][:, ::-1])
            assert np.array_equal(got.lo.cpu().numpy(), begin + rec["lo"][:, ::-1])
            assert np.array_equal(got.end.cpu().numpy(), begin + rec["hi"][:, ::-1] + 1)
            centroid = begin + (rec["sum"].astype(np.float64) / rec["voxels"].astype(np.float64)[:, None])[:, ::-1]
            assert np.allclose(got.centroid.cpu().numpy(), centroid, rtol=0, atol=1e-9)
            # the field the caller already holds gives the same bytes
            held = vol.distance(lod=lod, **kw)
            again = vol.split(distance=held, merge=merge, connectivity=connectivity)
            assert again.ids.cpu().numpy().tobytes() == got.ids.cpu().numpy().tobytes() and again.count == got.count
            for name in ("voxels", "region_basins", "peak_squared", "top", "lo", "end", "centroid"):
                assert getattr(again, name).cpu().numpy().tobytes() == getattr(got, name).cpu().numpy().tobytes(), (what, name)
            # the methods, from the twin's records
            scale = np.array(vol.wrapping_buffers[lod].scale_factor, np.float64)
            order = sorted(range(1, head[0] + 1), key=lambda k: (-int(rec["voxels"][k - 1]), k))
            assert got.largest(3) == order[:3] and got.largest(10 ** 6) == order
            for k in order[:3]:
                lo, end = begin + rec["lo"][k - 1][::-1], begin + rec["hi"][k - 1][::-1] + 1
                assert got.box(k) == (tuple(int(v) for v in np.floor(lo / scale)), tuple(int(v) for v in np.ceil(end / scale)))
                top = begin + rec["top"][k - 1][::-1]
                data = (top[::-1].astype(np.float64) + 0.5) / scale[::-1] - 0.5
                world = data * np.array([1.5, 0.5, 2.0]) + np.array([3.0, -2.0, 7.0])
                assert np.allclose(got.position(k), world, rtol=0, atol=1e-9)
                assert got.radius(k) == float(np.sqrt(float(rec["peak"][k - 1])))
                assert got.id_at(got.position(k)) == k
                assert np.array_equal(got.mask(k).cpu().numpy(), twin["ids"] == k)
            assert np.array_equal(got.mask(order[:2]).cpu().numpy(), np.isin(twin["ids"], order[:2]))
            assert got.id_at((-1e5, 0.0, 0.0)) == 0
        assert sum(n >= 3 for n, _ in counts) >= 3 and sum(b > n for n, b in counts) >= 3    # objects were split, and basins merged
        # two overlapping balls of one label: two regions until the merge is large
        off, shape, ring, dens, labs = window_of(vol, 0)
        pieces = [vol.split(labels=[1], merge=m).count for m in (0, 1.0, 100.0)]
        assert pieces[0] >= pieces[1] == 2 and pieces[2] == 1
        # an empty window: nothing to split
        empty = vol.split(level=LEVEL, box=((0, 0, 0), (4, 4, 4)))
        assert empty.count == 0 and empty.ids.numel() == 0 and empty.inside_voxels == 0 and len(empty) == 0 and empty.largest(3) == []
        none = vol.split(level=1e9)
        assert none.count == 0 and none.ids.numel() == int(np.prod(shape)) and not bool(none.ids.any())
        # another stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        again = vol.split(level=LEVEL, stream=side.cuda_stream)
        side.synchronize()
        want = split_twin(distance_twin(off, dens, labs, level=LEVEL, border=True)["d2"], 26, 1)
        assert np.array_equal(again.ids.cpu().numpy().view(np.uint32), want["ids"]) and again.count == want["header"][0]
    finally:
        vol.world.scale = (1.0, 1.0, 1.0)
        vol.world.position = (0.0, 0.0, 0.0)
