"""GPU: svr_upload_region, svr_upload_region_device and svr_read_region (include/svr.h) through the C entry points, with
the test's own strides and dtype codes, against the numpy model of tests/ring_transfer_cases.py.  Before every upload
the ring holds a known pattern without a zero in it; after it the WHOLE ring is read back and compared with the model
as bits (a NaN compares as NaN), so a voxel written beside the box shows as well as a wrong one inside it; where the
LOD keeps a micro-block copy, the copy is held to the ring.  Device sources are raw byte tensors seen through the dtype
code, so no torch dtype is needed; every pointer is a multiple of its element size."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ring_transfer_cases as RT
from sub_volume_renderer_amd import _native as N
from sub_volume_renderer_amd._wrapping_buffer import DeviceRings
from sub_volume_renderer_amd.testing import micro_blocks_of, read_micro_block_copy
from test_gpu_macro_cells import rows_per_block, staging_constants

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
CSRC = os.path.join(os.path.dirname(N.__file__), "csrc")
OK, INVALID, RANGE = 0, -1, -4                                          # SVR_OK, SVR_ERR_INVALID, SVR_ERR_RANGE
P = C.c_void_p
_fns = {}


def fn(name):
    """The entry point with every pointer as void*: NULL offsets, shapes and strides can be passed."""
    if name not in _fns:
        args = {"svr_read_region": [P, C.c_int, P, P, P, P]}.get(name, [P, C.c_int, P, P, P, C.c_int, P, P, C.c_int, P])
        _fns[name] = C.CFUNCTYPE(C.c_int, *args)((name, N.lib()))
    return _fns[name]


UPLOAD = {"host": "svr_upload_region", "device": "svr_upload_region_device"}


def last_error():
    return N.lib().svr_last_error().decode()


def byte_range(view):
    """[lo, hi): the bytes a strided view touches, relative to its element (0, 0, 0)."""
    lo = sum(min(0, s * (n - 1)) for s, n in zip(view.strides, view.shape))
    hi = sum(max(0, s * (n - 1)) for s, n in zip(view.strides, view.shape)) + view.itemsize
    return lo, hi


class Rig:
    """One context with one LOD, its numpy model, and the pattern both start from."""

    def __init__(self, ring_zyx, storage="float32", labels=True, fill=True):
        self.shape = tuple(ring_zyx)
        self.dtype = {"float32": F32, "uint8": np.uint8, "uint16": np.uint16}[storage]
        self.has_labels = labels
        self.rings = DeviceRings([self.shape], density_storage=storage, labels=labels)
        self.keep = []                                                  # device sources, until the next read-back
        self.model = RT.RingModel(self.shape, self.dtype, labels)
        if fill:
            self.reset()

    def reset(self):
        """A full-ring upload of the pattern."""
        d, lab = RT.pattern(self.shape, self.dtype, self.has_labels)
        assert self.send("host", (0, 0, 0), d, lab) == OK, last_error()
        self.hold("pattern")

    def device_ptr(self, view, align=0):
        lo, hi = byte_range(view)
        pad = (align + lo) % 16                                         # element (0, 0, 0) lands `align` bytes past a 16-byte boundary
        raw = np.frombuffer(C.string_at(view.ctypes.data + lo, hi - lo), np.uint8).copy()
        t = torch.zeros(pad + hi - lo, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        t[pad:] = torch.from_numpy(raw).cuda()
        self.keep.append(t)
        return t.data_ptr() + pad - lo

    def send(self, path, off_xyz, density=None, labels=None, *, align=0):
        """One upload of [z][y][x] views with the strides they have; the model follows when the call succeeds."""
        shape_xyz = (density if density is not None else labels).shape[::-1]
        args = []
        for src in (density, labels):
            if src is None:
                args += [None, 0, None]
            else:
                where = src.ctypes.data if path == "host" else self.device_ptr(src, align)
                assert where % src.itemsize == 0
                args += [where, N.dtype_code(src.dtype), N.l3(src.strides[::-1])]
        rc = fn(UPLOAD[path])(self.rings.handle, 0, N.i3(off_xyz), N.i3(shape_xyz), *args)
        if rc == OK:
            self.model.upload(off_xyz, density, labels)
        return rc

    def read(self, off_xyz=(0, 0, 0), shape_xyz=None):
        shape_xyz = self.shape[::-1] if shape_xyz is None else shape_xyz
        d = np.full(shape_xyz[::-1], -5.0, F32)
        lab = np.full(shape_xyz[::-1], 0xABCDEF01, U32)
        rc = fn("svr_read_region")(self.rings.handle, 0, N.i3(off_xyz), N.i3(shape_xyz), d.ctypes.data, lab.ctypes.data)
        assert rc == OK, last_error()
        self.keep.clear()                                               # the read-back waited for the upload stream
        return d, lab

    def hold(self, msg=""):
        """The whole ring == the model, bit for bit; the micro-block copy == the ring."""
        d, lab = self.read()
        want = self.model.density
        if self.dtype == F32:
            same = (d.view(U32) == want.view(U32)) | (np.isnan(d) & np.isnan(want))
        else:
            same = d == want.astype(F32)
        assert same.all(), f"{msg}: density differs at (z, y, x) {np.argwhere(~same)[:6].tolist()} of {np.count_nonzero(~same)}"
        if self.has_labels:
            diff = lab != self.model.labels
            assert not diff.any(), f"{msg}: labels differ at (z, y, x) {np.argwhere(diff)[:6].tolist()} of {np.count_nonzero(diff)}"
        else:
            assert not lab.any(), f"{msg}: a context without label rings reads labels as 0"
        twin = read_micro_block_copy(self.rings, 0)
        if twin is not None:
            raw = {1: np.uint8, 2: np.uint16, 4: U32}[twin.dtype.itemsize]
            np.testing.assert_array_equal(twin.view(raw), micro_blocks_of(d.astype(self.dtype)).view(raw),
                                          err_msg=f"{msg}: micro-block copy")
        return twin is not None

    def close(self):
        self.keep.clear()
        self.rings.close()


_rigs = {}


def rig(ring_zyx=(8, 8, 48), storage="float32", labels=True):
    """Shared small contexts: every test puts the pattern back before its upload."""
    key = (tuple(ring_zyx), storage, labels)
    if key not in _rigs:
        _rigs[key] = Rig(ring_zyx, storage, labels, fill=False)
    _rigs[key].reset()
    return _rigs[key]


# ---- 1. casts --------------------------------------------------------------------------------------------------------
BOX_ZYX, OFF_XYZ = (5, 3, 19), (21, 2, 1)                               # off every 16-voxel boundary, inside the 8 x 8 x 48 ring
N_BOX = 5 * 3 * 19


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("dtype", RT.DTYPES, ids=lambda d: np.dtype(d).name)
def test_casts_are_numpys(dtype, path):
    r = rig()
    d = RT.density_values(dtype, N_BOX, 11).reshape(BOX_ZYX)
    lab = RT.label_values(dtype, N_BOX, 11).reshape(BOX_ZYX)
    assert r.send(path, OFF_XYZ, d, lab) == OK, last_error()
    assert r.hold(f"{np.dtype(dtype).name} {path}")                     # (this ring keeps a micro-block copy)
    box = r.model.box(OFF_XYZ, BOX_ZYX[::-1])
    assert np.count_nonzero(r.model.density[box] != RT.pattern(r.shape, F32)[0][box]) > N_BOX // 2


@pytest.mark.parametrize("path", ["host", "device"])
def test_native_rings_take_their_own_type(path):
    for storage, sources in (("uint8", [RT.density_values(np.uint8, N_BOX, 5), np.arange(N_BOX) % 3 == 0]),
                             ("uint16", [RT.density_values(np.uint16, N_BOX, 5)])):
        for src in sources:                                             # (bool travels as code 0, one byte per voxel)
            r = rig(storage=storage)
            assert r.send(path, OFF_XYZ, src.reshape(BOX_ZYX), RT.label_values(np.int16, N_BOX, 5).reshape(BOX_ZYX)) == OK, last_error()
            assert r.hold(f"{storage} {src.dtype} {path}")


# ---- 2. strides ------------------------------------------------------------------------------------------------------
def strided_views(dtype, seed):
    z, y, x = BOX_ZYX
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    full = rng.integers(info.min, info.max, (z, y, 3 * x), dtype=dtype, endpoint=True)
    box = np.ascontiguousarray(full[:, :, :x])
    return {"flip_x": box[:, :, ::-1], "flip_y": box[:, ::-1, :], "flip_z": box[::-1], "flip_all": box[::-1, ::-1, ::-1],
            "third_x": full[:, :, ::3], "one_row": np.broadcast_to(box[:, :1, :], BOX_ZYX),
            "one_plane": np.broadcast_to(box[:1], BOX_ZYX)}


STRIDE_KINDS = ["flip_x", "flip_y", "flip_z", "flip_all", "third_x", "one_row", "one_plane"]


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("kind", STRIDE_KINDS)
def test_negative_zero_and_wide_strides(kind, path):
    d, lab = strided_views(np.int16, 1)[kind], strided_views(np.uint64, 2)[kind]
    assert d.shape == lab.shape == BOX_ZYX
    sx, sy, sz = d.strides[::-1]
    assert {"flip_x": sx < 0, "flip_y": sy < 0, "flip_z": sz < 0, "flip_all": sx < 0 and sy < 0 and sz < 0,
            "third_x": sx == 6, "one_row": sy == 0, "one_plane": sz == 0}[kind]
    r = rig()
    assert r.send(path, OFF_XYZ, d, lab) == OK, last_error()
    r.hold(f"{kind} {path}")


# ---- 3. which scatter kernel runs ------------------------------------------------------------------------------------
def test_the_conditions_of_the_streaming_path_are_the_ones_broken_below():
    text = open(os.path.join(CSRC, "ring_kernels.hip")).read()
    for line in ("(a.density_dtype == a.ring_storage && a.dstride[0] == des && aligned16(a.src_density) &&",
                 "a.dstride[1] % 16 == 0 && a.dstride[2] % 16 == 0);",
                 "((a.labels_dtype == SVR_U32 || a.labels_dtype == SVR_I32) && a.lstride[0] == 4 && aligned16(a.src_labels) &&",
                 "a.lstride[1] % 16 == 0 && a.lstride[2] % 16 == 0);",
                 "const bool geo_ok = (a.shape[0] & 15) == 0 && (a.dst_off[0] & 15) == 0 && (a.ring[0] & 15) == 0 &&"):
        assert line in text, "svr_launch_scatter chooses its kernel differently now: revisit the cases of this file"


@pytest.mark.parametrize("storage", ["uint8", "uint16", "float32"])
def test_streaming_box_and_each_condition_broken_alone(storage):
    """Ring x = 48, box x = 32 at x = 16, packed rows, 16-byte-aligned sources of the ring's own type with u32 labels:
    the streaming kernel (16-byte loads and stores).  Then one condition at a time is broken, which sends the box to
    the per-voxel kernel (or, for i32 labels and a flipped y, still streams).  Either way the ring equals the model
    inside the box and around it: a 16-byte store that spilled onto a neighbour would show there."""
    dt = {"uint8": np.uint8, "uint16": np.uint16, "float32": F32}[storage]
    rng = np.random.default_rng(21)

    def density(shape, dtype=dt):
        return RT.density_values(dtype, int(np.prod(shape)), int(rng.integers(1 << 30))).reshape(shape)

    def labels(shape, dtype=U32):
        return RT.label_values(dtype, int(np.prod(shape)), int(rng.integers(1 << 30))).reshape(shape)

    base = (2, 3, 32)
    cases = [                                                            # name, ring x, offset, density, labels, align, paths
        ("streams", 48, (16, 2, 1), density(base), labels(base), 0, "both"),
        ("box x 31", 48, (16, 2, 1), density((2, 3, 31)), labels((2, 3, 31)), 0, "both"),
        ("box x 33", 48, (0, 2, 1), density((2, 3, 33)), labels((2, 3, 33)), 0, "both"),
        ("offset x 8", 48, (8, 2, 1), density(base), labels(base), 0, "both"),
        ("ring x 40", 40, (0, 2, 1), density(base), labels(base), 0, "both"),
        ("source + 4 bytes", 48, (16, 2, 1), density(base), labels(base), 4, "device"),
        ("i32 labels", 48, (16, 2, 1), density(base), labels(base, np.int32), 0, "both"),
        ("i64 labels", 48, (16, 2, 1), density(base), labels(base, np.int64), 0, "both"),
        ("density only", 48, (16, 2, 1), density(base), None, 0, "both"),
        ("labels only", 48, (16, 2, 1), None, labels(base), 0, "both"),
        ("flipped y", 48, (16, 2, 1), density(base)[:, ::-1, :], labels(base)[:, ::-1, :], 0, "device"),
        ("one row for all", 48, (16, 2, 1), np.broadcast_to(density((2, 1, 32)), base), np.broadcast_to(labels((2, 1, 32)), base), 0, "device"),
    ]
    if storage == "uint8":
        cases.append(("row stride 36 bytes", 48, (16, 2, 1), density((2, 3, 36))[:, :, :32], labels(base), 0, "device"))
    if storage == "float32":
        cases.append(("f64 density", 48, (16, 2, 1), density(base, np.float64), labels(base), 0, "both"))
    for name, ring_x, off, d, lab, align, paths in cases:
        for path in (("host", "device") if paths == "both" else (paths,)):
            r = rig((8, 8, ring_x), storage)
            assert r.send(path, off, d, lab, align=align) == OK, (name, last_error())
            assert r.hold(f"{storage} {name} {path}")                   # both rings keep a micro-block copy


# ---- 4. the staged blocks of a host upload ---------------------------------------------------------------------------
def test_staged_blocks_whole_planes_and_runs_of_rows():
    """f64 density and i64 labels, 16 bytes per voxel, into a 4 x 512 x 528 float ring.  A box of 2 x 300 x 500 travels
    as two blocks of one plane each (the second at a z offset); two whole planes of the ring travel as runs of rows
    inside a plane (blocks at non-zero y and z offsets).  Both from the constants of svr_upload.hip."""
    ring = (4, 512, 528)
    r = Rig(ring)
    rng = np.random.default_rng(31)

    def sources(shape):
        return rng.standard_normal(shape) * 1e3, rng.integers(-2**63, 2**63 - 1, shape, dtype=np.int64)

    planes = (2, 300, 500)
    per_block, plane = rows_per_block(planes, 16)
    assert plane <= per_block < 2 * plane                               # one whole plane per block, two blocks
    d, lab = sources(planes)
    assert r.send("host", (5, 100, 2), d, lab) == OK, last_error()
    assert r.hold("whole planes")
    rows = (2, 512, 528)
    per_block, plane = rows_per_block(rows, 16)
    assert per_block < plane and plane % per_block                      # runs of rows, the last one of a plane shorter
    d, lab = sources(rows)
    assert r.send("host", (0, 0, 1), d, lab) == OK, last_error()
    r.hold("runs of rows")
    r.close()


# ---- 5. more voxels than one pass of the capped grid -----------------------------------------------------------------
@pytest.mark.parametrize("storage", ["uint8", "uint16", "float32"])
def test_second_pass_of_the_capped_grid(storage):
    """A 96 x 96 x 80 ring, 737,280 voxels against the 2048 x 256 = 524,288 threads of one pass of grid_for: the read-back
    of the whole ring takes a second pass on every storage; on the float ring so does one per-voxel scatter (an f64 / i64
    device source)."""
    text = open(os.path.join(CSRC, "ring_kernels.hip")).read()
    assert "const size_t cap = 256 * 8;" in text, "the grid cap of ring_kernels.hip changed: resize this ring"
    ring = (80, 96, 96)
    assert 2048 * 256 < int(np.prod(ring)) < 2 * 2048 * 256
    r = Rig(ring, storage)                                              # pattern up, whole ring read back and held
    if storage == "float32":
        rng = np.random.default_rng(41)
        d, lab = rng.standard_normal(ring) * 1e3, rng.integers(-2**63, 2**63 - 1, ring, dtype=np.int64)
        assert r.send("device", (0, 0, 0), d, lab) == OK, last_error()
        r.hold("one scatter of the whole ring")
    r.close()


# ---- 6. the read-back itself -----------------------------------------------------------------------------------------
def special_ring(storage):
    """(rig, density as float32, labels): 255 / 65535 / the non-finite table at slot 0, at the last slot and between."""
    r = rig(storage=storage)
    top = {"uint8": [255, 0, 254], "uint16": [65535, 0, 256], "float32": RT.DENSITY_EDGES[np.float32]}[storage]
    d = r.model.density.copy()
    flat = d.reshape(-1)
    flat[:len(top)] = top
    flat[-len(top):] = top[::-1]
    flat[1000:1000 + len(top)] = top
    lab = r.model.labels.copy()
    lab.reshape(-1)[[0, -1]] = 0xFFFFFFFF, 0x80000000
    assert r.send("host", (0, 0, 0), d, lab) == OK, last_error()
    return r, d.astype(F32), lab


@pytest.mark.parametrize("storage", ["uint8", "uint16", "float32"])
def test_read_region_boxes(storage):
    r, d, lab = special_ring(storage)
    z, y, x = r.shape
    for off, shape in (((0, 0, 0), (1, 1, 1)), ((x - 1, y - 1, z - 1), (1, 1, 1)), ((0, 0, 0), (x, y, z)), ((5, 3, 2), (17, 4, 5)),
                       ((x - 3, y - 2, z - 1), (3, 2, 1))):
        box = r.model.box(off, shape)
        gd, gl = r.read(off, shape)
        np.testing.assert_array_equal(gd.view(U32), d[box].view(U32), err_msg=f"{storage} {off} {shape}")
        np.testing.assert_array_equal(gl, lab[box])
    assert d.reshape(-1)[0] in (255, 65535) or np.isnan(d.reshape(-1)[0])
    # one output NULL: the other is filled, and a NULL one is nobody's to write
    read = fn("svr_read_region")
    off, shape = (5, 3, 2), (17, 4, 5)
    box = r.model.box(off, shape)
    gd, gl = np.full(shape[::-1], -5.0, F32), np.full(shape[::-1], 0xABCDEF01, U32)
    assert read(r.rings.handle, 0, N.i3(off), N.i3(shape), None, gl.ctypes.data) == OK
    np.testing.assert_array_equal(gl, lab[box])
    assert np.all(gd == -5.0)
    gl[:] = 0xABCDEF01
    assert read(r.rings.handle, 0, N.i3(off), N.i3(shape), gd.ctypes.data, None) == OK
    np.testing.assert_array_equal(gd.view(U32), d[box].view(U32))
    assert np.all(gl == 0xABCDEF01)
    gd[:] = -5.0
    assert read(r.rings.handle, 0, N.i3(off), N.i3(shape), None, None) == OK
    for axis in range(3):                                               # an empty box writes nothing
        empty = list(shape)
        empty[axis] = 0
        assert read(r.rings.handle, 0, N.i3(off), N.i3(empty), gd.ctypes.data, gl.ctypes.data) == OK
        edge = [0, 0, 0]
        edge[axis] = r.shape[::-1][axis]                                # offset == extent with nothing to read: inside
        assert read(r.rings.handle, 0, N.i3(edge), N.i3(empty), gd.ctypes.data, gl.ctypes.data) == OK
    assert np.all(gd == -5.0) and np.all(gl == 0xABCDEF01)


def test_read_region_without_label_rings():
    r = rig(labels=False)
    d = RT.density_values(np.float32, N_BOX, 3).reshape(BOX_ZYX)
    assert r.send("device", OFF_XYZ, d) == OK, last_error()
    r.hold("label-less")                                                # labels read 0, density intact
    lab = np.full(BOX_ZYX, 0xABCDEF01, U32)
    assert fn("svr_read_region")(r.rings.handle, 0, N.i3(OFF_XYZ), N.i3(BOX_ZYX[::-1]), None, lab.ctypes.data) == OK
    assert not lab.any()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_ring_alone():
    r = rig()
    x, y, z = r.shape[::-1]
    d32 = RT.density_values(np.float32, 8, 1).reshape(2, 2, 2)
    l32 = RT.label_values(np.uint32, 8, 1).reshape(2, 2, 2)
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    gd, gl = np.full((2, 2, 2), -5.0, F32), np.full((2, 2, 2), 0xABCDEF01, U32)
    st4, st8 = N.l3((4, 8, 16)), N.l3((8, 16, 32))
    big = 2**31 - 1

    def regions():
        """(off, shape, code, text) for every region check_region refuses"""
        yield None, (2, 2, 2), INVALID, "null argument"
        yield (0, 0, 0), None, INVALID, "null argument"
        for axis in range(3):
            ring = (x, y, z)[axis]
            for off, n in ((-1, 2), (0, -1), (ring - 1, 2), (ring + 1, 0), (big, 2), (0, ring + 1)):
                o, s = [0, 0, 0], [2, 2, 2]
                o[axis], s[axis] = off, n
                yield tuple(o), tuple(s), RANGE, "region outside the ring"

    def vec(v):
        return None if v is None else N.i3(v)

    for path, name in UPLOAD.items():
        src_d, src_l = (d32.ctypes.data, l32.ctypes.data) if path == "host" else (dev.data_ptr(), dev.data_ptr() + 32)
        up = fn(name)

        def call(handle=r.rings.handle, lod=0, off=(1, 1, 1), shape=(2, 2, 2), d=src_d, dcode=8, dst=st4, lab=src_l, lcode=2, lst=st4):
            return up(handle, lod, vec(off), vec(shape), d, dcode, dst, lab, lcode, lst)

        refused = [(dict(handle=None), INVALID, "null argument"), (dict(lod=-1), INVALID, "lod out of range"),
                   (dict(lod=1), INVALID, "lod out of range")]
        refused += [(dict(off=o, shape=s), code, text) for o, s, code, text in regions()]
        refused += [(dict(dcode=-1), INVALID, "bad density dtype/strides"), (dict(dcode=10), INVALID, "bad density dtype/strides"),
                    (dict(lcode=-1), INVALID, "bad labels dtype/strides"), (dict(lcode=10), INVALID, "bad labels dtype/strides"),
                    (dict(dst=None), INVALID, "bad density dtype/strides"), (dict(lst=None), INVALID, "bad labels dtype/strides")]
        for kw, code, text in refused:
            assert call(**kw) == code, (name, kw, last_error())
            assert f"{name}: {text}" in last_error(), (name, kw, last_error())
        r.hold(f"after the refusals of {name}")
    read = fn("svr_read_region")

    def read_call(handle=r.rings.handle, lod=0, off=(1, 1, 1), shape=(2, 2, 2)):
        return read(handle, lod, vec(off), vec(shape), gd.ctypes.data, gl.ctypes.data)

    refused = [(dict(handle=None), INVALID, "null argument"), (dict(lod=-1), INVALID, "lod out of range"),
               (dict(lod=1), INVALID, "lod out of range")]
    refused += [(dict(off=o, shape=s), code, text) for o, s, code, text in regions()]
    for kw, code, text in refused:
        assert read_call(**kw) == code, (kw, last_error())
        assert f"svr_read_region: {text}" in last_error(), (kw, last_error())
    assert np.all(gd == -5.0) and np.all(gl == 0xABCDEF01)
    assert read_call() == OK and not np.any(gd == -5.0)
    # what a context cannot take: labels without label rings, a foreign type into an integer ring
    cannot = [(rig(labels=False), F32, "created without label rings (no_labels)", dict(labels=True)),
              (rig(storage="uint8"), np.uint16, "integer density storage only accepts sources of that same dtype", {}),
              (rig(storage="uint8"), F32, "integer density storage only accepts sources of that same dtype", {}),
              (rig(storage="uint16"), np.uint8, "integer density storage only accepts sources of that same dtype", {})]
    for rr, dt, text, extra in cannot:
        for path, name in UPLOAD.items():
            d = RT.density_values(dt, N_BOX, 2).reshape(BOX_ZYX)
            lab = RT.label_values(np.uint16, N_BOX, 2).reshape(BOX_ZYX) if (extra or rr.has_labels) else None
            assert rr.send(path, OFF_XYZ, d, lab) == INVALID, (name, dt)
            assert f"{name}: " in last_error() and text in last_error(), last_error()
            rr.hold(f"after {name} refused {np.dtype(dt).name}")
        own = RT.density_values(rr.dtype, N_BOX, 2).reshape(BOX_ZYX)     # the control upload
        assert rr.send("host", OFF_XYZ, own, RT.label_values(np.uint16, N_BOX, 2).reshape(BOX_ZYX) if rr.has_labels else None) == OK
        rr.hold("control")
    for path in UPLOAD:                                                 # the control uploads of the first ring
        assert r.send(path, (1, 1, 1), d32, l32) == OK, last_error()
        r.hold(f"control {path}")


def test_a_row_as_wide_as_a_staging_slot():
    """f64 + i64 sources, 16 bytes per voxel: a row of kStagingSlotBytes - 32 bytes is staged and lands intact, one voxel
    more is refused and leaves the ring as it was."""
    slot, _, _ = staging_constants()
    fits = (slot - 32) // 16
    assert fits == 3145726
    r = Rig((1, 1, 3145728))
    rng = np.random.default_rng(51)
    d, lab = rng.standard_normal((1, 1, fits + 1)), rng.integers(-2**63, 2**63 - 1, (1, 1, fits + 1), dtype=np.int64)
    assert r.send("host", (1, 0, 0), d[:, :, 1:], lab[:, :, 1:]) == OK, last_error()
    r.hold("the widest row")
    assert r.send("host", (1, 0, 0), d, lab) == INVALID
    assert "svr_upload_region: one row of the region exceeds the staging slot" in last_error()
    r.hold("after the refusal")
    assert r.send("device", (1, 0, 0), d, lab) == OK, last_error()      # a device source is not staged
    r.hold("control")
    r.close()
