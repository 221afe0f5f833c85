"""GPU: svr_pool2x and write_multiscale_store against oracle/pool_oracle.py, everything compared as bits (f32 through a
uint32 view, NaN against NaN): every x remainder of the u8 kernel's groups of four, long thin volumes, base pointers at
every byte offset (u8) and at an odd element offset (f32 / u32: copied by pool2x, refused by the C entry point), the
second pass of the capped grid for all three kernels, the value cases of test_pyramid.py (hand-derived there), and
stores written in several slabs with ragged shards."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import pool_oracle
from sub_volume_renderer_amd import _native as N, zarr3
from sub_volume_renderer_amd.pyramid import pool2x, write_multiscale_store
from test_pyramid import bits, f32_value_cases, oracle_pyramid, row_of_blocks, u8_value_cases, u32_value_cases

pytestmark = pytest.mark.gpu

GRID_CAP_THREADS = 256 * 16 * 256                    # threads of one pass of a pool kernel's grid (pool_kernels.hip)
KINDS = {"u8": (np.uint8, "mean", pool_oracle.mean_u8, N.SVR_U8, 0), "f32": (np.float32, "mean", pool_oracle.mean_f32, N.SVR_F32, 0),
         "u32": (np.uint32, "max", pool_oracle.max_u32, 2, 1)}


def fill(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "f32":
        return (rng.random(shape) * 300 - 20).astype(np.float32)
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint32)


def to_dev(a):
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(t, kind):
    a = t.cpu().numpy()
    return a.view(np.uint32) if kind == "u32" else a


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan)                           # NaN against NaN, whatever its payload
        np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])
    else:
        np.testing.assert_array_equal(got, want)


def pooled(a, kind):
    return to_host(pool2x(to_dev(a), KINDS[kind][1]), kind)


SHAPES = [(z, y, x) for x in (2, 6, 8, 10, 14, 18, 30, 64) for y in (2, 6) for z in (2, 6)] + \
         [(2, 2, 8192), (2, 8192, 2), (8192, 2, 2)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_x_remainder_and_long_thin_volumes(kind):
    """ox = 1, 3, 4, 5, 7, 9, 15, 32: every count the u8 kernel's last group of four can hold, with and without full
    groups before it; 8192 along each axis alone."""
    for i, shape in enumerate(SHAPES):
        a = fill(kind, shape, 100 + i)
        same_bits(pooled(a, kind), KINDS[kind][2](a))


@pytest.mark.parametrize("x", [16, 20])
def test_u8_at_every_byte_offset(x):
    """The u8 kernel takes its 8-byte path row by row from the row's address: rows of 16 bytes keep the alignment of the
    base (fast at offset 0 only), rows of 20 alternate between two alignments (some rows fast, some not, at offsets 0 and
    4).  The destination is a fresh tensor and, in a second round, a view at byte offsets 1 .. 3 between sentinels."""
    shape = (4, 6, x)
    n = int(np.prod(shape))
    a = fill("u8", shape, 7)
    want = pool_oracle.mean_u8(a)
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    for off in range(8):
        view = buf[off:off + n].view(shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 8 == off and view.is_contiguous()
        rows = (view.data_ptr() + x * np.arange(shape[0] * shape[1])) % 8 == 0
        assert rows.any() == (off == 0 or (x == 20 and off == 4)) and (x == 16 or not rows.all())
        np.testing.assert_array_equal(pool2x(view, "mean").cpu().numpy(), want)
        out = torch.full((want.size + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        doff = 1 + off % 3
        dims = N.i3(shape[::-1])
        assert N.lib().svr_pool2x(0, C.c_void_p(view.data_ptr()), C.c_void_p(out.data_ptr() + doff), dims, N.SVR_U8, 0, None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[doff:doff + want.size].reshape(want.shape), want)
        assert (got[:doff] == 0xA5).all() and (got[doff + want.size:] == 0xA5).all()


@pytest.mark.parametrize("kind", ["f32", "u32"])
def test_odd_element_offset_is_copied_by_pool2x_and_refused_by_the_c_call(kind):
    shape = (6, 10, 14)
    n = int(np.prod(shape))
    a = fill(kind, shape, 9)
    want = KINDS[kind][2](a)
    buf = torch.zeros(n + 4, dtype=to_dev(a).dtype, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[1:1 + n].view(shape)
    view.copy_(to_dev(a))
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    same_bits(to_host(pool2x(view, KINDS[kind][1]), kind), want)
    # the raw entry point decides on the host, before any launch
    lib = N.lib()
    out = torch.full((want.size + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dims, code, mode = N.i3(shape[::-1]), KINDS[kind][3], KINDS[kind][4]
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)                           # noqa: E731
    for src, dst, msg in ((p(view), p(out), "src must be 8-byte aligned"), (p(buf, 2), p(out), "src must be 8-byte aligned"),
                          (p(buf), p(out, 2), "dst must be 4-byte aligned"), (p(buf), p(out, 1), "dst must be 4-byte aligned"),
                          (None, p(out), "null argument"), (p(buf), None, "null argument")):
        assert lib.svr_pool2x(0, src, dst, dims, code, mode, None) == -1, msg
        assert ("svr_pool2x: " + msg) in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all())
    # the control case: the same data from an aligned address, and a dst that is 4- but not 8-byte aligned
    aligned = view.clone()
    assert aligned.data_ptr() % 8 == 0 and (out.data_ptr() + 4) % 8 == 4
    assert lib.svr_pool2x(0, p(aligned), p(out, 4), dims, code, mode, None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    same_bits(got[1:1 + want.size].view(want.dtype).reshape(want.shape), want)
    assert got[0] == 0x5A5A5A5A and (got[1 + want.size:] == 0x5A5A5A5A).all()


@pytest.mark.parametrize("kind,shape", [("f32", (132, 256, 256)), ("u32", (132, 256, 256)), ("u8", (132, 256, 1024))])
def test_second_pass_of_the_capped_grid(kind, shape):
    """1,081,344 threads against a grid of 4096 x 256 = 1,048,576: the last 32,768 are reached by the grid-stride step."""
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "pool_kernels.hip")).read()
    assert "if (blocks > 256 * 16) blocks = 256 * 16;" in src, "the grid cap of pool_kernels.hip changed: resize these volumes"
    z, y, x = (s // 2 for s in shape)
    threads = z * y * (-(-x // 4) if kind == "u8" else x)
    assert threads == 1_081_344 and GRID_CAP_THREADS == 1_048_576 < threads < 2 * GRID_CAP_THREADS
    a = fill(kind, shape, 21)
    same_bits(pooled(a, kind), KINDS[kind][2](a))


def test_value_cases():
    """The blocks of test_pyramid.py (hand-derived there), side by side along x and, for u8, shifted by one block so
    that every case meets every lane of the group of four."""
    names, blocks, want = zip(*f32_value_cases())
    got = pooled(row_of_blocks(blocks, np.float32), "f32")[0, 0]
    for n, g, w in zip(names, got, want):
        assert (np.isnan(g) and np.isnan(w)) or bits(np.float32(g).reshape(1))[0] == bits(np.float32(w).reshape(1))[0], (n, g, w)
    same_bits(pooled(row_of_blocks(blocks, np.float32), "f32"), pool_oracle.mean_f32(row_of_blocks(blocks, np.float32)))
    names, blocks, want = zip(*u8_value_cases())
    for shift in range(4):
        row = list(blocks[shift:]) + list(blocks[:shift])
        exp = list(want[shift:]) + list(want[:shift])
        np.testing.assert_array_equal(pooled(row_of_blocks(row, np.uint8), "u8")[0, 0], np.asarray(exp, np.uint8))
    names, blocks, want = zip(*u32_value_cases())
    np.testing.assert_array_equal(pooled(row_of_blocks(blocks, np.uint32), "u32")[0, 0], np.asarray(want, np.uint32))
    # whole volumes of the extremes
    np.testing.assert_array_equal(pooled(np.full((6, 6, 30), 255, np.uint8), "u8"), np.full((3, 3, 15), 255, np.uint8))
    np.testing.assert_array_equal(pooled(np.zeros((6, 6, 30), np.uint32), "u32"), np.zeros((3, 3, 15), np.uint32))
    np.testing.assert_array_equal(pooled(np.full((6, 6, 30), 0xFFFFFFFF, np.uint32), "u32"), np.full((3, 3, 15), 0xFFFFFFFF, np.uint32))


def test_python_surface_refuses_what_it_documents():
    with pytest.raises(TypeError):
        pool2x(torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"), "max")     # max takes int32 only
    with pytest.raises(TypeError):
        pool2x(torch.zeros((4, 4, 4), dtype=torch.int32, device="cuda"), "mean")
    with pytest.raises(ValueError):
        pool2x(torch.zeros((4, 4, 8), dtype=torch.float32, device="cuda")[:, :, ::2], "mean")
    with pytest.raises(ValueError):
        pool2x(torch.zeros((4, 4, 6), dtype=torch.float32, device="cuda")[:, :, :5], "mean")
    assert "int32" in pool2x.__doc__ and "or uint8" not in pool2x.__doc__


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", [(96, 48, 80), (128, 32, 32)], ids=["ragged", "whole_slabs"])
def test_write_multiscale_store_across_slab_seams(tmp_path, kind, shape):
    """Chunks of 8^3 in shards of 16^3, three levels: slabs of 64 planes.  (96, 48, 80) is a slab of 64 planes and one of
    32, whose level 2 is 8 planes, half a shard, and whose extents at every level are no multiples of the shard;
    (128, 32, 32) is two whole slabs.  Every level read back equals the pyramid of the WHOLE array pooled on the CPU:
    pooling slab by slab must land where pooling the whole would."""
    dtype, mode = KINDS[kind][0], KINDS[kind][1]
    a = fill(kind, shape, 31)
    levels = 3
    arrays = write_multiscale_store(str(tmp_path / "s.zarr"), a, levels, mode, chunks=(8, 8, 8), shards=(16, 16, 16))
    assert -(-shape[0] // (16 << (levels - 1))) == 2                                # two slabs
    want = oracle_pyramid(a, levels, mode)
    assert sorted(zarr3.open_group(str(tmp_path / "s.zarr")).keys()) == ["scale0", "scale1", "scale2"]
    for k in range(levels):
        assert arrays[k].shape == tuple(s >> k for s in shape) and arrays[k].dtype == np.dtype(dtype)
        assert arrays[k].chunks == (8, 8, 8) and arrays[k].shards == (16, 16, 16)
        same_bits(np.asarray(arrays[k][:, :, :]), want[k])
