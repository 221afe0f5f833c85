"""GPU: the macro-cell maxima behind empty-space skipping (svr_lod_cell_ptrs, include/svr.h), read back and held to the
numpy restatement testing.macro_cells_of over the ring as it lies in HBM — EXACTLY, after every step: walks of wrapped
loads through the streaming and the general scatter, overwrites that make maxima go down, single voxels at the slots
where a refresh range can be one cell short, blocks staged as runs of rows inside one plane, coarser LODs, a LOD without
a grid, clears, asynchronous window moves.  A table that is too high costs only speed and one that is too low is seen by
a frame only where a ray happens to cross: neither shows in the frame tests.  Last, that the march and the iso kernel
really read the tables this accessor returns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sub_volume_renderer_amd import Coordinate, Roi, WrappingBuffer, _native as N
from sub_volume_renderer_amd._wrapping_buffer import DeviceRings
from sub_volume_renderer_amd.testing import macro_cell_bytes, macro_cells_of, read_macro_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = [np.uint8, np.uint16, np.float32]
NAME = {np.uint8: "uint8", np.uint16: "uint16", np.float32: "float32"}
BRIGHT = {np.uint8: 200, np.uint16: 40000, np.float32: -7.5}         # above 127, above 32767, negative


# ---- reading and comparing ------------------------------------------------------------------------------------------
def read_ring(rings, lod):
    """The density ring of one LOD [z][y][x] in its own element type (svr_read_region hands out float32: exact for all three)."""
    shape = rings.ring_shapes[lod]
    out = np.empty(shape, np.float32)
    N.check(N.lib().svr_read_region(rings.handle, lod, N.i3((0, 0, 0)), N.i3(shape[::-1]), C.c_void_p(out.ctypes.data), None),
            "svr_read_region")
    return out.astype({"uint8": np.uint8, "uint16": np.uint16}.get(rings.density_storage, np.float32))


def hold_tables(rings, lod, what, ring=None):
    """Both tables of one LOD against the restatement over the ring's contents.  -> (ring, raw, blk)"""
    ring = read_ring(rings, lod) if ring is None else ring
    cshift = macro_cell_bytes(rings, lod)[4]
    assert cshift == (3 if lod == 0 else 2), (what, cshift)
    raw, blk = read_macro_cells(rings, lod)
    want_raw, want_blk = macro_cells_of(ring, cshift)
    assert raw.shape == want_raw.shape and raw.dtype == ring.dtype, (what, raw.shape, raw.dtype)
    # the safety half (a table that is too low skips occupied space): blk >= raw >= |slot|
    s = 1 << cshift
    mag = np.abs(ring) if ring.dtype.kind == "f" else ring
    slots_raw = np.repeat(np.repeat(np.repeat(raw, s, 0), s, 1), s, 2)
    assert not np.any(mag > slots_raw), f"{what}: raw TOO LOW at {int(np.count_nonzero(mag > slots_raw))} slots"
    assert not np.any(raw > blk), f"{what}: blk TOO LOW (below raw) at cells {np.argwhere(raw > blk)[:8].tolist()}"
    for d in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1)):
        assert not np.any(np.roll(raw, tuple(-v for v in d), (0, 1, 2)) > blk), f"{what}: blk TOO LOW (below the raw cell at +{d})"
    assert not np.isnan(raw).any() and not np.isnan(blk).any(), what
    # the other half (too high: only speed is lost, no frame test sees it), and with it equality
    np.testing.assert_array_equal(raw, want_raw, err_msg=f"{what}: raw differs; TOO HIGH at {int(np.count_nonzero(raw > want_raw))} cells")
    np.testing.assert_array_equal(blk, want_blk, err_msg=f"{what}: blk differs; TOO HIGH at {int(np.count_nonzero(blk > want_blk))} cells")
    return ring, raw, blk


def upload(rings, lod, off_zyx, block, device=False):
    """One svr_upload_region (host) or svr_upload_region_device (a torch tensor) of a density block [z][y][x], no labels."""
    off, shape = N.i3(tuple(off_zyx)[::-1]), N.i3(tuple(block.shape)[::-1])
    none = (None, 0, N.l3((0, 0, 0)))
    if device:
        strides = N.l3([s * block.element_size() for s in block.stride()][::-1])
        code = N.dtype_code(np.dtype(str(block.dtype).replace("torch.", "")))
        N.check(N.lib().svr_upload_region_device(rings.handle, lod, off, shape, C.c_void_p(block.data_ptr()), code, strides, *none),
                "svr_upload_region_device")
    else:
        N.check(N.lib().svr_upload_region(rings.handle, lod, off, shape, C.c_void_p(block.ctypes.data), N.dtype_code(block.dtype),
                                          N.l3(block.strides[::-1]), *none), "svr_upload_region")


def clear(rings, lod):
    N.check(N.lib().svr_clear_lod(rings.handle, lod), "svr_clear_lod")


# ---- walks of wrapped loads -------------------------------------------------------------------------------------------
WALK_SHAPE = (96, 80, 160)
WALK_OFFSETS = ((0, 0, 0), (8, 4, 16), (40, 36, 80), (70, 60, 130), (33, 27, 51), (0, 0, 0))
WALK_BUFFERS = (((4, 4, 16), (6, 6, 4)), ((2, 2, 4), (12, 12, 16)))      # chunk x ring in chunks: both rings 24 x 24 x 64 (z, y, x)
WALK_SEED, WALK_COUNT = 24, 200


def walk_volume(dtype):
    """A dark volume (zeros) with WALK_COUNT isolated bright voxels, two in three of them on a corner or a face of the 8^3
    cells (the rings' extents are multiples of 8: a voxel's place inside its cell is the same in the ring); float32: every
    other bright value negative, and a few NaN, one +inf and one -0.0 beside them."""
    rng = np.random.default_rng(WALK_SEED)
    data = np.zeros(WALK_SHAPE, dtype)
    hi = {np.uint8: 255, np.uint16: 65535, np.float32: 1000}[dtype]
    for k in range(WALK_COUNT):
        p = np.array([rng.integers(0, n) for n in WALK_SHAPE])
        if k % 3 == 0:
            p = np.minimum((p // 8) * 8 + rng.choice([0, 7], 3), np.array(WALK_SHAPE) - 1)     # a cell corner
        elif k % 3 == 1:
            a = (k // 3) % 3
            p[a] = min((p[a] // 8) * 8 + int(rng.choice([0, 7])), WALK_SHAPE[a] - 1)             # a cell face
        v = int(rng.integers(hi // 2, hi)) + 1                                                 # u8 > 127, u16 > 32767
        data[tuple(p)] = -v if (dtype == np.float32 and k % 2) else v
    if dtype == np.float32:
        for k in range(40):
            data[tuple(rng.integers(0, n) for n in WALK_SHAPE)] = np.nan
        data[3, 5, 7], data[2, 9, 40], data[1, 1, 1] = np.inf, -0.0, np.nan                    # inside the first window, as is
        data[8:16, 8:16, 16:24] = np.nan                                                       # a cell of nothing but NaN
    return data


def walk_wants(ring_px, chunk):
    return [tuple(min(r - c, s - o) for r, c, s, o in zip(ring_px, chunk, WALK_SHAPE, off)) for off in WALK_OFFSETS]


@pytest.mark.parametrize("dtype", STORAGES, ids=lambda d: np.dtype(d).name)
def test_tables_follow_the_ring_through_wrapped_loads(dtype):
    """Chunk-aligned loads through the 16-voxel streaming scatter and loads off the 16-voxel and the cell grid through the
    per-voxel scatter, windows that wrap around the ring, slots of chunks that left the window: exact after every load."""
    data = walk_volume(dtype)
    for chunk, ring in WALK_BUFFERS:
        buf = WrappingBuffer(data, None, Coordinate(ring), Coordinate(chunk))
        assert buf.rings.density_storage == NAME[dtype]
        ring_px = tuple(int(v) for v in buf.shape_in_pixels)
        assert ring_px == (24, 24, 64)
        for k, (off, want) in enumerate(zip(WALK_OFFSETS, walk_wants(ring_px, chunk))):
            buf.load_logical_roi(Roi(off, want))
            tex, raw, blk = hold_tables(buf.rings, 0, (np.dtype(dtype).name, chunk, off))
            if k:
                # (worked out from the restatement alone, tests/test_cell_range.py holds that to hand-made answers: the
                # comparison above had empty blocks, occupied blocks and blocks lit only by a neighbour to tell apart)
                want_raw, want_blk = macro_cells_of(tex, 3)
                assert np.count_nonzero(want_blk == 0) >= 10 and np.count_nonzero(want_blk) >= 10, (chunk, off, want_blk.tolist())
                assert np.any(want_raw != want_blk)
            if dtype == np.float32 and k == 0:
                assert np.isnan(tex).any() and np.isinf(tex).any() and np.signbit(tex[tex == 0]).any()
        clear(buf.rings, 0)
        _, raw, blk = hold_tables(buf.rings, 0, "cleared")
        assert not raw.any() and not blk.any()
        buf.rings.close()


# ---- maxima go down -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", STORAGES, ids=lambda d: np.dtype(d).name)
def test_maxima_go_down_when_bright_slots_are_overwritten(dtype):
    rings = DeviceRings([(16, 16, 32)], density_storage=NAME[dtype], labels=False)        # cdim (z, y, x) = (2, 2, 4)
    rng = np.random.default_rng(5)
    data = rng.integers(100, 120, (16, 16, 32)).astype(dtype)
    peak = {np.uint8: 255, np.uint16: 65535, np.float32: -300.0}[dtype]
    data[1, 2, 3] = peak                                      # the one largest |value| of the ring, in cell (0, 0, 0)
    data[5, 5, 6] = 130 if dtype != np.float32 else -130.0    # what cell (0, 0, 0) falls back to: in the half that stays
    upload(rings, 0, (0, 0, 0), data)
    _, raw, blk = hold_tables(rings, 0, "bright")
    top = abs(peak)
    held = [(z, y, x) for z in (0, 1) for y in (0, 1) for x in (0, 3)]       # the blocks that hold cell (0, 0, 0): cdim - 1 and 0
    assert raw[0, 0, 0] == top and all(blk[c] == top for c in held) and np.count_nonzero(blk == top) == 8
    upload(rings, 0, (0, 0, 0), np.zeros((8, 8, 4), dtype))   # half of cell (0, 0, 0), reaching slot 0 on x
    ring, raw, blk = hold_tables(rings, 0, "half a cell overwritten with zeros")
    assert not ring[:8, :8, :4].any()
    assert raw[0, 0, 0] == 130 and np.count_nonzero(raw == top) == 0
    assert all(blk[c] == 130 for c in held), blk.tolist()     # ... also the blocks that start at the last cell on x
    rings.close()


# ---- single voxels through the ABI --------------------------------------------------------------------------------------
def lit_blocks(cell, cdim):
    """The cells (z, y, x) whose 2 x 2 x 2 block holds `cell`: c - 1 and c per axis, on the torus."""
    return {((cell[0] - a) % cdim[0], (cell[1] - b) % cdim[1], (cell[2] - c) % cdim[2]) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


@pytest.mark.parametrize("dtype", STORAGES, ids=lambda d: np.dtype(d).name)
def test_single_voxels_into_a_cleared_ring(dtype):
    """One voxel at slot 0 (its blocks start at the LAST cell), at the last slot of the first cell, at the first of the
    second, and at the ring's last slot; cells of 8^3 (LOD 0) and 4^3 (LOD 1)."""
    rings = DeviceRings([(24, 24, 32), (16, 24, 8)], density_storage=NAME[dtype], labels=False)
    v = np.full((1, 1, 1), BRIGHT[dtype], dtype)
    for lod, s in ((0, 8), (1, 4)):
        shape = rings.ring_shapes[lod]
        cdim = tuple(n // s for n in shape)
        assert min(cdim) >= 2 and max(cdim) >= 3
        for slot in ((0, 0, 0), (s - 1, s - 1, s - 1), (s, s, s), tuple(n - 1 for n in shape)):
            clear(rings, lod)
            upload(rings, lod, slot, v)
            ring, raw, blk = hold_tables(rings, lod, (lod, slot))
            cell = tuple(p // s for p in slot)
            assert np.count_nonzero(ring) == 1 and ring[slot] == v[0, 0, 0]
            assert {tuple(c) for c in np.argwhere(raw)} == {cell} and raw[cell] == abs(BRIGHT[dtype])
            assert {tuple(c) for c in np.argwhere(blk)} == lit_blocks(cell, cdim), (lod, slot, np.argwhere(blk).tolist())
            assert np.all(blk[blk != 0] == abs(BRIGHT[dtype]))
    rings.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", STORAGES, ids=lambda d: np.dtype(d).name)
def test_single_voxels_into_a_ring_one_cell_wide(dtype, device):
    """A ring of 8 x 8 x 16 slots has 1 x 1 x 2 cells: every block wraps onto itself on y and z and holds both cells on x."""
    import torch

    rings = DeviceRings([(8, 8, 16)], density_storage=NAME[dtype], labels=False)
    big = np.zeros((3, 4, 7), dtype)
    big[1, 2, 4] = BRIGHT[dtype]
    src = torch.from_numpy(big).cuda()[1:2, 2:3, 4:5] if device else big[1:2, 2:3, 4:5]      # strided, one element
    for slot in ((0, 0, 0), (7, 7, 7), (0, 0, 8), (7, 7, 15)):
        clear(rings, 0)
        upload(rings, 0, slot, src, device)
        ring, raw, blk = hold_tables(rings, 0, (slot, device))
        assert ring[slot] == BRIGHT[dtype] and np.count_nonzero(ring) == 1
        want = [0, 0]
        want[slot[2] // 8] = abs(BRIGHT[dtype])
        assert raw.tolist() == [[want]] and blk.tolist() == [[[abs(BRIGHT[dtype])] * 2]]
    rings.close()


# ---- staged blocks that are runs of rows inside one plane ---------------------------------------------------------------
def staging_constants():
    """(slot bytes, smallest block bytes, blocks per region) as svr_upload.hip names them."""
    text = open(os.path.join(ROOT, "sub_volume_renderer_amd", "csrc", "svr_upload.hip")).read()

    def const(name):
        m = re.search(r"static const size_t %s = (?:\(size_t\))?(\d+)(?: << (\d+))?;" % name, text)
        assert m, name
        return int(m.group(1)) << int(m.group(2) or 0)

    assert "std::min(c->slot_bytes - 32, std::max<size_t>(kMinBlockBytes, region_bytes / kBlocksPerRegion))" in text
    return const("kStagingSlotBytes"), const("kMinBlockBytes"), const("kBlocksPerRegion")


def rows_per_block(shape_zyx, bytes_per_voxel):
    """How svr_upload_region cuts a region: (rows a staged block may hold, rows of one plane)."""
    slot, least, parts = staging_constants()
    row = shape_zyx[2] * bytes_per_voxel
    block = min(slot - 32, max(least, row * shape_zyx[1] * shape_zyx[0] // parts))
    return max(1, block // row), shape_zyx[1]


def test_blocks_that_are_runs_of_rows_inside_one_plane():
    """A float32 ring with labels, 8 x 544 x 976 slots: 8 bytes per voxel, 7808 per row, 4.05 MiB per plane.  A block is
    max(smallest block, region / 8) bytes.  With the whole ring in one call that is one plane exactly (a grid needs extents
    that are multiples of 8, so a ring's eighth is never less than a plane: whole planes, first step).  Four planes in one
    call make it the smallest block, 4 MiB = 537 rows < 544: every plane travels as a run of 537 rows and one of 7, and
    the cells of rows 536 .. 543 are refreshed by both (second step).  Both derived below from the constants of
    svr_upload.hip, so a change there fails here rather than quietly leaving the row path untested."""
    shape = (8, 544, 976)
    rng = np.random.default_rng(9)
    assert rows_per_block(shape, 8)[0] >= shape[1]                            # the whole ring: whole planes
    per_block, plane = rows_per_block((4, *shape[1:]), 8)
    assert per_block < plane and per_block % 8 and plane % per_block, (per_block, plane)      # four planes: runs of rows, cut inside a cell
    rings = DeviceRings([shape], density_storage="float32", labels=True)

    def sparse(z):
        wide = np.zeros((z, shape[1], 2 * shape[2]), np.float32)
        at = tuple(rng.integers(0, n, 600) for n in wide.shape)
        wide[at] = rng.standard_normal(600).astype(np.float32) * 100.0
        wide[:, per_block - 1, 0], wide[:, per_block, 2] = 7000.0, -9000.0     # either side of the cut between two runs, one cell
        return wide[:, :, ::2]                                                 # strided host data

    def send(z0, block):
        labels = np.ones(block.shape, np.uint32)
        N.check(N.lib().svr_upload_region(rings.handle, 0, N.i3((0, 0, z0)), N.i3(block.shape[::-1]), C.c_void_p(block.ctypes.data),
                                          N.dtype_code(block.dtype), N.l3(block.strides[::-1]), C.c_void_p(labels.ctypes.data),
                                          N.dtype_code(labels.dtype), N.l3(labels.strides[::-1])), "svr_upload_region")

    first = sparse(8)
    send(0, first)
    ring, raw, blk = hold_tables(rings, 0, "whole planes")
    np.testing.assert_array_equal(ring, first)
    for z0 in (0, 4):
        send(z0, sparse(4))
    ring, raw, blk = hold_tables(rings, 0, "runs of rows")
    assert np.count_nonzero(ring != first) > 100 and raw[0, (per_block - 1) // 8, 0] == 9000.0
    assert np.count_nonzero(blk == 0) >= 10 and np.any(raw != blk)
    rings.close()


# ---- coarser LODs, a LOD without a grid, clears, streaming ----------------------------------------------------------------
def hold_volume(vol, what, expect_none=()):
    out = []
    for lod, buf in enumerate(vol.wrapping_buffers):
        if lod in expect_none:
            assert read_macro_cells(vol._rings, lod) is None and macro_cell_bytes(vol._rings, lod) is None, (what, lod)
            continue
        out.append(hold_tables(vol._rings, lod, (what, lod)))
    return out


@pytest.mark.parametrize("storage,dtype,scale", [("native", np.uint8, 1), ("float32", np.uint8, 1), ("native", np.uint16, 257)])
def test_every_lod_through_window_moves_and_label_uploads(storage, dtype, scale):
    """Three LODs (8^3 cells at LOD 0, 4^3 at LODs 1 and 2), eight window moves, blocking and asynchronous in turn: exact
    once the uploads have landed.  An upload of labels alone leaves the tables as they are."""
    from sub_volume_renderer_amd import testing
    from test_gpu_skip import _scene, _sparse_pairs

    pairs = [(d.astype(dtype) * scale, l) for d, l in _sparse_pairs(128, 3, count=120, noise=2)]
    spec = _scene(128, pairs, 180.0 * scale, "K2", storage)
    vol = testing.build(spec).volume
    assert [tuple(r) for r in vol._rings.ring_shapes] == [(48, 48, 48), (48, 48, 48), (32, 32, 32)]
    before = hold_volume(vol, "first load")
    assert all(np.count_nonzero(blk) > 0 and np.any(raw != blk) for _, raw, blk in before)
    eye = np.array(spec.cam_position)
    d = np.array(spec.cam_target) - eye
    d = d / np.linalg.norm(d)
    changed = 0
    for k in range(1, 9):
        vol.center_on_position(tuple(eye + d * 7.0 * k), asynchronous=bool(k & 1))
        vol.poll_uploads(wait=True)
        after = hold_volume(vol, ("move", k))
        changed += sum(int(not np.array_equal(a[0], b[0])) for a, b in zip(after, before))
        before = after
    assert changed >= 4                                         # the moves did rewrite ring slots
    labels = np.full((16, 16, 16), 9, np.uint32)
    for lod in range(3):
        N.check(N.lib().svr_upload_region(vol._rings.handle, lod, N.i3((8, 4, 0)), N.i3((16, 16, 16)), None, 0, N.l3((0, 0, 0)),
                                          C.c_void_p(labels.ctypes.data), N.dtype_code(labels.dtype), N.l3(labels.strides[::-1])),
                "svr_upload_region")
    for (ring0, raw0, blk0), (ring1, raw1, blk1) in zip(before, hold_volume(vol, "labels alone")):
        assert np.array_equal(raw0, raw1) and np.array_equal(blk0, blk1) and np.array_equal(ring0, ring1, equal_nan=True)
    vol.close()


def test_a_lod_without_a_grid_and_cleared_lods():
    """A LOD whose ring is 44 slots on one axis has no tables (null pointers); the LODs around it are exact.  svr_clear_lod
    zeroes both tables, and the next load is exact again."""
    from sub_volume_renderer_amd import testing
    from test_gpu_skip import _sparse_pairs

    pairs = _sparse_pairs(128, 4, count=60, noise=2)
    spec = testing.synthetic_spec(128, 96, 64, pairs=pairs, chunk_shapes=[(8, 8, 16), (4, 4, 16), (2, 2, 16)],
                                  ring_shapes=[(6, 6, 3), (11, 12, 3), (16, 16, 2)])
    vol = testing.build(spec).volume
    assert [tuple(r) for r in vol._rings.ring_shapes] == [(48, 48, 48), (44, 48, 48), (32, 32, 32)]
    held = hold_volume(vol, "first load", expect_none=(1,))
    assert len(held) == 2 and all(np.count_nonzero(blk) > 0 for _, _, blk in held)
    for lod in (0, 2):
        clear(vol._rings, lod)
        ring, raw, blk = hold_tables(vol._rings, lod, ("cleared", lod))
        assert not ring.any() and not raw.any() and not blk.any()
    vol.center_on_position((40.0, 44.0, 50.0))                 # loads the chunks that are new to each window, into zeros
    held = hold_volume(vol, "load after the clear", expect_none=(1,))
    assert np.count_nonzero(held[0][2]) > 0                     # (the coarsest ring holds its whole level: nothing new to load)
    vol.close()


# ---- the kernels read these tables ----------------------------------------------------------------------------------------
def _skip_scene():
    from sub_volume_renderer_amd import testing
    from test_gpu_skip import _scene, _sparse_pairs

    spec = _scene(128, _sparse_pairs(128, 2), 150.0, "K1")
    scene = testing.build(spec)
    return spec, scene, [macro_cell_bytes(scene.volume._rings, lod) for lod in range(3)]


def test_the_march_reads_these_tables():
    """blk of every LOD filled with the type's maximum through the returned pointers: nothing can be skipped any more, the
    LMIP frame is the skip-off frame bit for bit with no skipped batch in the census (with the true tables: > 1000)."""
    import torch

    from sub_volume_renderer_amd import testing

    spec, scene, tables = _skip_scene()
    vol, cam, w, h = scene.volume, scene.camera, spec.width, spec.height
    handle = vol._rings.handle
    census = (C.c_uint32 * 8)()
    planes = ("rgba", "depth", "label", "flags", "steps")

    def lmip_frame(variant):
        N.check(N.lib().svr_set_variant(handle, variant), "svr_set_variant")
        N.check(N.lib().svr_debug_counters(handle, census, 1), "svr_debug_counters")
        _, inst = testing.render_both(vol, cam, w, h)
        frame = {k: getattr(inst, k).clone() for k in planes}
        N.check(N.lib().svr_debug_counters(handle, census, 1), "svr_debug_counters")
        N.check(N.lib().svr_set_variant(handle, 0), "svr_set_variant")
        return frame, int(census[7])

    off, skipped_off = lmip_frame(8)                            # bit 3: no skipping
    on, skipped_on = lmip_frame(0)
    assert skipped_off == 0 and skipped_on > 1000
    assert all(t is not None for t in tables)
    for _, blk, _, dt, _ in tables:
        assert dt == np.uint8
        blk.fill_(255)                                          # the type's maximum
    torch.cuda.synchronize()
    full, skipped_full = lmip_frame(0)
    vol.close()                                                 # its tables are wrong now: never rendered from again
    for k in planes:
        assert torch.equal(full[k], off[k]), k
    assert skipped_full == 0


def _covered_scene():
    """A test_gpu_skip-style scene (dark volume, bright blobs, three LODs, the same chunk shapes) made so that the tables
    decide every sample that can hit:
    - every LOD's window holds its whole level (rings of 128^3, 64^3, 32^3 slots, windows as large, offset 0): no point of
      the volume lies outside every window, where the iso kernel passes stretches without asking a table, and every sample
      resolves at LOD 0 in one span per ray without a ring wrap;
    - the march tests cells only while a wave's run has >= 4 * skip_batches batches left (march_kernel.hip), and a run ends
      where the first live lane's ray ends: what a wave fetches whatever blk holds lies within 32 iterations before the
      exit of its shortest ray and the exits of its others.  The camera looks down +x from outside and the 6^3 blobs sit
      at x < 41, 40 .. 88 in y and z: at least 87 voxels (108 iterations) before the exit face x = 128 and, at the
      <= 17 degrees a ray of this camera makes with the axis, more than 110 before a side face."""
    from sub_volume_renderer_amd import testing

    n = 128
    rng = np.random.default_rng(6)
    d0, l0 = np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint32)
    for k in range(14):
        z, y, x = int(rng.integers(40, 83)), int(rng.integers(40, 83)), int(rng.integers(12, 35))
        d0[z:z + 6, y:y + 6, x:x + 6] = 200
        l0[z:z + 6, y:y + 6, x:x + 6] = 1 + k
    pairs, d, l = [(d0, l0)], d0, l0
    for _ in range(2):
        m = d.shape[0] // 2
        d = (d.reshape(m, 2, m, 2, m, 2).astype(np.uint32).sum(axis=(1, 3, 5)) // 8).astype(np.uint8)
        l = l.reshape(m, 2, m, 2, m, 2).max(axis=(1, 3, 5))
        pairs.append((d, l))
    sizes = [(128,) * 3, (64,) * 3, (32,) * 3]
    spec = testing.synthetic_spec(n, 192, 128, pairs=pairs, chunk_shapes=[(8, 8, 16), (4, 4, 16), (2, 2, 16)],
                                  ring_shapes=[(16, 16, 8), (16, 16, 4), (16, 16, 2)])
    spec.material.update(lmip_threshold=150.0, clim=(0.0, 255.0))
    spec.centers = [((64.0, 64.0, 64.0), sizes)]
    c = (n - 1) / 2.0
    view = np.array((-1.0, 0.01, 0.02)) / np.linalg.norm((-1.0, 0.01, 0.02))
    spec.cam_position, spec.cam_target = tuple(np.array([c, c, c]) + 1.7 * n * view), (c, c, c)
    inside = testing.synthetic_spec(n, 192, 128, inside=True, pairs=pairs).camera()
    scene = testing.build(spec)
    for lod, buf in enumerate(scene.volume.wrapping_buffers):
        roi = buf._current_logical_roi_in_pixels
        assert tuple(roi.offset) == (0, 0, 0) and tuple(roi.shape) == sizes[lod] == tuple(scene.volume._rings.ring_shapes[lod])
    return spec, scene, inside, [macro_cell_bytes(scene.volume._rings, lod) for lod in range(3)]


def test_the_iso_kernel_reads_these_tables_and_zeroed_tables_hide_every_hit():
    """With blk of every LOD at the type's maximum the iso frame is the no_skip frame bit for bit with no skipped stretch
    (with the true tables: thousands).  With blk of every LOD zeroed the LMIP frame has no hit left where
    the oracle, and the frame from the true tables, have more than 100.  The scene: _covered_scene.  (In the scene of
    test_the_march_reads_these_tables neither holds, for reasons that are not the tables': 323 of 7474 iso stretches lie
    outside every window, and its 5 hit pixels are sampled in runs too short to be tested.)"""
    import torch

    from oracle import lmip
    from test_gpu_iso import assert_same_planes, both_ways, iso_on

    spec, scene, inside, tables = _covered_scene()
    vol, cam, w, h = scene.volume, scene.camera, spec.width, spec.height
    assert all(t is not None for t in tables)
    true_flags = vol.render(cam, w, h, count_steps=True).flags.cpu().numpy()
    mode = vol.material.render_mode
    iso_on(vol, 150.0, iso_refine=5)
    (_, n_true), _ = both_ways(vol, inside, w, h)
    for _, blk, _, _, _ in tables:
        blk.fill_(255)
    torch.cuda.synchronize()
    (iso_full, n_full), (iso_off, n_off) = both_ways(vol, inside, w, h)
    print("iso wave-stretches marched / skipped: true tables", n_true, "blk at the maximum", n_full, "no_skip", n_off)
    vol.material.render_mode = mode
    for _, blk, _, _, _ in tables:
        blk.zero_()
    torch.cuda.synchronize()
    empty = vol.render(cam, w, h, count_steps=True)
    torch.cuda.synchronize()
    ref = lmip.render_scene(scene)
    hits = int(np.count_nonzero(ref.flags == 2)), int(np.count_nonzero(true_flags == 2)), int((empty.flags == 2).sum())
    print("LMIP hits: oracle, true tables, blk zeroed", hits)
    vol.close()                                                 # its tables are wrong now: never rendered from again
    assert n_true[1] > 1000 and n_true[0] + n_true[1] == n_off[0]      # the true tables do pass stretches
    assert_same_planes(iso_full, iso_off, "blk at the maximum")
    assert n_full[1] == 0 and n_off[1] == 0 and n_full[0] == n_off[0] > 0
    assert np.array_equal(true_flags, ref.flags) and hits[0] > 100
    assert hits[2] == 0
