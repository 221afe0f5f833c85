"""Value tables and the numpy model of a ring upload (svr_upload_region / svr_upload_region_device, include/svr.h):
`texture.data[box] = np.array(src, float32 | uint32)`.  tests/test_ring_transfer.py holds the model to bits written by
hand; tests/test_gpu_ring_transfer.py holds the scatter kernels and the read-back to the model.

The tables hold, per source dtype, the values at which a cast goes wrong: rounding ties of wide integers to f32, f64
values that overflow, go subnormal or round to even, negative integers that wrap into labels, 64-bit labels at and
beyond 2^32, float labels that truncate toward zero.  Float labels stay inside [0, 2^32): the header leaves the rest
undefined."""
import numpy as np

F32, U32 = np.float32, np.uint32

DTYPES = [np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]   # code order

DENSITY_EDGES = {
    np.uint8: [0, 255], np.uint16: [0, 65535], np.int8: [-128, 127], np.int16: [-32768, 32767],
    np.uint32: [2**24 + 1, 2**31 + 64, 2**31 + 192, 2**32 - 1],
    np.int32: [-2**31, 2**31 - 1, -(2**24) - 1],
    np.uint64: [2**24 + 1, 2**24 + 3, 2**53 + 1, 2**63, 2**64 - 1, 2**40 + 2**16],
    np.int64: [-2**63, 2**63 - 1, -(2**24) - 3],
    np.float32: [np.nan, np.inf, -np.inf, -0.0, 1e-41, 3.4028234663852886e38],
    np.float64: [1e39, -1e39, 1e-40, 1e-46, -0.0, 1 + 2.0**-24, 1 + 2.0**-24 + 2.0**-50, 1 + 3 * 2.0**-24,
                 3.4028235677973366e38, np.nan, np.inf, -np.inf],
}

FLOAT_LABELS = [0.0, 0.999, 1.5, 16777217.0, 4294967040.0, 2.0**31 + 0.5]      # (as f32: 16777216 and 2^31)
LABEL_EDGES = {
    np.uint8: [0, 255], np.uint16: [0, 65535], np.uint32: [0, 2**32 - 1],
    np.int8: [-128, 127, -1], np.int16: [-32768, 32767, -1], np.int32: [-2**31, 2**31 - 1, -1],
    np.uint64: [0, 2**64 - 1, 2**32, 2**32 + 5, 2**40 + 7, 2**63 - 1],
    np.int64: [-2**63, 2**63 - 1, -1, 2**32, 2**32 + 5, 2**40 + 7],
    np.float32: FLOAT_LABELS, np.float64: FLOAT_LABELS + [4294967295.9],       # (as f32 that one is 2^32: outside)
}


def _fill(dtype, n, rng, labels):
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if labels:                                                          # inside [0, 2^32), fractions included
        return np.minimum(rng.random(n) * 2.0**32, 4294967040.0).astype(dt)
    return (rng.standard_normal(n) * 1000.0).astype(dt)


def density_values(dtype, n, seed=0):
    """n values of `dtype`: its edge table, then a seeded fill over the type's whole range."""
    edges = np.array(DENSITY_EDGES[dtype], dtype=dtype)
    assert len(edges) <= n
    return np.concatenate([edges, _fill(dtype, n - len(edges), np.random.default_rng(seed), False)])


def label_values(dtype, n, seed=0):
    edges = np.array(LABEL_EDGES[dtype], dtype=dtype)
    assert len(edges) <= n
    return np.concatenate([edges, _fill(dtype, n - len(edges), np.random.default_rng(seed + 1), True)])


def cast_density(src):
    """numpy's cast to float32 (round to nearest even; f64 beyond the f32 range goes to inf, that is the cast)."""
    with np.errstate(over="ignore"):
        return np.array(src, dtype=F32)


def cast_labels(src):
    """numpy's cast to uint32: integers wrap modulo 2^32, floats in [0, 2^32) truncate toward zero."""
    return np.asarray(src).astype(U32)


class RingModel:
    """A ring as numpy arrays [z][y][x]: density in the ring's element type, labels u32 (or None)."""

    def __init__(self, shape_zyx, dtype=F32, labels=True):
        self.density = np.zeros(shape_zyx, dtype)
        self.labels = np.zeros(shape_zyx, U32) if labels else None

    def box(self, off_xyz, shape_xyz):
        return tuple(slice(o, o + n) for o, n in zip(off_xyz[::-1], shape_xyz[::-1]))

    def upload(self, off_xyz, density=None, labels=None):
        """model[box] = cast(src); sources are [z][y][x] views of any strides."""
        for src in (density, labels):
            if src is not None:
                shape_xyz = src.shape[::-1]
        if density is not None:
            cast = cast_density(density) if self.density.dtype == F32 else np.asarray(density).astype(self.density.dtype)
            self.density[self.box(off_xyz, shape_xyz)] = cast
        if labels is not None:
            self.labels[self.box(off_xyz, shape_xyz)] = cast_labels(labels)


def pattern(shape_zyx, dtype, labels=True):
    """A known pattern without a zero in it: (density in the ring's type, labels)."""
    i = np.arange(int(np.prod(shape_zyx)), dtype=np.uint64).reshape(shape_zyx)
    d = (i * np.uint64(7) % np.uint64(251) + np.uint64(1)).astype(dtype)
    if np.dtype(dtype) == F32:
        d = (d + F32(0.25)).astype(F32)
    lab = ((i * np.uint64(2654435761)) % np.uint64(2**32)).astype(U32) | U32(1) if labels else None
    return d, lab
