"""The numpy model of a ring upload (tests/ring_transfer_cases.py) against bits written by hand: what `np.array(src,
float32)` and `.astype(uint32)` give at the values where a cast can go wrong, and that the model places a cast box and
leaves the rest alone.  tests/test_gpu_ring_transfer.py holds the scatter kernels to this model."""
import numpy as np
import pytest

import ring_transfer_cases as RT

F32, U32 = np.float32, np.uint32

F32_BITS = [                                # source dtype, value, bits of the float32
    (np.uint64, 2**24 + 1, 0x4B800000),     # tie, to even (down)
    (np.uint64, 2**24 + 3, 0x4B800002),     # tie, to even (up)
    (np.uint64, 2**53 + 1, 0x5A000000),
    (np.uint64, 2**63, 0x5F000000),
    (np.uint64, 2**64 - 1, 0x5F800000),     # rounds up to 2^64
    (np.int64, -2**63, 0xDF000000),
    (np.uint32, 2**32 - 1, 0x4F800000),
    (np.uint32, 2**31 + 64, 0x4F000000),    # spacing 256 above 2^31: the nearer neighbour is below
    (np.uint32, 2**31 + 192, 0x4F000001),   # ... and above
    (np.float64, 1e39, 0x7F800000),         # beyond the f32 range: inf
    (np.float64, 1e-40, 0x000116C2),        # a subnormal f32
    (np.float64, 1e-46, 0x00000000),        # below half the smallest subnormal
    (np.float64, -0.0, 0x80000000),
    (np.float64, 1 + 2.0**-24, 0x3F800000),                 # tie, to even
    (np.float64, 1 + 2.0**-24 + 2.0**-50, 0x3F800001),      # just above the tie
    (np.float64, 1 + 3 * 2.0**-24, 0x3F800002),             # tie, to even (up)
]
U32_LABELS = [                              # source dtype, value, the uint32 label
    (np.int8, -128, 4294967168),
    (np.int64, 2**32 + 5, 5),
    (np.int64, -2**63, 0),
    (np.uint64, 2**32, 0),
    (np.uint64, 2**64 - 1, 4294967295),
    (np.float32, 4294967040.0, 4294967040),
    (np.float64, 4294967295.9, 4294967295),
]


@pytest.mark.parametrize("dtype, value, want", F32_BITS, ids=lambda v: getattr(v, "__name__", None) or repr(v))
def test_density_cast_bits(dtype, value, want):
    src = np.array([value], dtype=dtype)
    assert RT.cast_density(src).view(U32)[0] == want
    assert value in RT.DENSITY_EDGES[dtype] or (value != value)          # the GPU tier uploads this very value


@pytest.mark.parametrize("dtype, value, want", U32_LABELS, ids=lambda v: getattr(v, "__name__", None) or repr(v))
def test_label_cast_values(dtype, value, want):
    src = np.array([value], dtype=dtype)
    got = RT.cast_labels(src)
    assert got.dtype == U32 and int(got[0]) == want
    assert value in RT.LABEL_EDGES[dtype]


def test_uint32_tie_at_spacing_256_is_what_the_table_says():
    # 2^31 + 64 and + 192 are no ties (the spacing above 2^31 is 256): they round to the nearer neighbour; the tie
    # 2^31 + 128 goes to the even mantissa, 2^31
    assert RT.cast_density(np.array([2**31 + 128], np.uint32)).view(U32)[0] == 0x4F000000
    assert RT.cast_density(np.array([2**31 + 129], np.uint32)).view(U32)[0] == 0x4F000001


def test_tables_cover_every_dtype_and_their_extremes():
    assert set(RT.DENSITY_EDGES) == set(RT.LABEL_EDGES) == set(RT.DTYPES)
    for dt in (np.uint8, np.uint16, np.int8, np.int16):
        info = np.iinfo(dt)
        assert {info.min, info.max} <= set(RT.DENSITY_EDGES[dt]) and {info.min, info.max} <= set(RT.LABEL_EDGES[dt])
    for dt in (np.int8, np.int16, np.int32, np.int64):
        assert -1 in RT.LABEL_EDGES[dt]
        assert RT.cast_labels(np.array([-1], dt))[0] == 0xFFFFFFFF
    for dt in (np.float32, np.float64):
        v = np.array(RT.LABEL_EDGES[dt], dt)
        assert np.all((v >= 0) & (v < 2.0**32))
        assert RT.cast_labels(v).tolist() == [0, 0, 1, 16777216 if dt == np.float32 else 16777217,
                                              4294967040, 2**31] + ([] if dt == np.float32 else [4294967295])
    for dt in RT.DTYPES:
        n = 285
        d, lab = RT.density_values(dt, n, 3), RT.label_values(dt, n, 3)
        assert d.dtype == lab.dtype == np.dtype(dt) and len(d) == len(lab) == n
        assert d[:len(RT.DENSITY_EDGES[dt])].tobytes() == np.array(RT.DENSITY_EDGES[dt], dt).tobytes()
        if np.dtype(dt).kind == "f":
            assert np.all((lab >= 0) & (lab < 2.0**32)) and np.any(lab != np.floor(lab))
        elif np.dtype(dt).kind == "i":
            assert np.any(d < 0) and np.any(lab < 0)                    # negative sources wrap into labels
    nan = RT.cast_density(np.array(RT.DENSITY_EDGES[np.float64]))
    assert np.isnan(nan[9]) and np.isposinf(nan[[0, 8, 10]]).all() and np.isneginf(nan[[1, 11]]).all()


def test_model_places_a_cast_box_and_leaves_the_rest():
    ring = RT.RingModel((4, 5, 6))
    d0, l0 = RT.pattern((4, 5, 6), F32)
    assert np.all(d0 != 0) and np.all(l0 != 0)
    ring.upload((0, 0, 0), d0, l0)
    src = np.arange(2 * 3 * 4, dtype=np.int16).reshape(2, 3, 4) - 12
    ring.upload((1, 2, 1), density=src[::-1, :, ::-1], labels=src)
    want_d, want_l = d0.copy(), l0.copy()
    for z in range(2):
        for y in range(3):
            for x in range(4):
                want_d[1 + z, 2 + y, 1 + x] = float(src[1 - z, y, 3 - x])
                want_l[1 + z, 2 + y, 1 + x] = int(src[z, y, x]) % 2**32
    np.testing.assert_array_equal(ring.density, want_d)
    np.testing.assert_array_equal(ring.labels, want_l)
    ring.upload((0, 0, 0), labels=np.broadcast_to(np.array([7, 8, 9, 10, 11, 12], np.uint64) + np.uint64(2**32), (4, 5, 6)))
    np.testing.assert_array_equal(ring.density, want_d)
    assert ring.labels[3, 4].tolist() == [7, 8, 9, 10, 11, 12]
    bytes_ring = RT.RingModel((2, 2, 8), np.uint8, labels=False)
    bytes_ring.upload((2, 0, 1), density=np.array([[[True, False, True]]]))
    assert bytes_ring.density[1, 0].tolist() == [0, 0, 1, 0, 1, 0, 0, 0] and bytes_ring.labels is None
