"""numpy restatement of svr_distance (include/svr.h): the exact squared Euclidean distance, in voxels, of every target of
the box B of one LOD's resident window to the nearest source, with the header.  ``squared_edt`` works on the box alone
(arrays [z][y][x]): three per-axis minima of g[i] + (u - i)^2, every line against every position of the line, in int64.
``distance_twin`` cuts the box out of a window and decides inside() with the lines of ``components_twin`` (the CPU test
holds the two to one another), swaps targets and sources for ``invert``, adds the border term and the header.  No scipy in
here: the CPU test holds this file to ``scipy.ndimage.distance_transform_edt``."""
import numpy as np

f32 = np.float32
FAR = 0x7FFFFFFF
NONE = np.int64(1) << 60               # "no source yet": larger than every sum of three squares, and it does not overflow


def axis_minimum(g, axis):
    """out[.., u, ..] = min over i of g[.., i, ..] + (u - i)^2 along ``axis``; g int64."""
    n = g.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    u = np.arange(n, dtype=np.int64).reshape(shape)
    out = np.full(g.shape, NONE, np.int64)
    for i in range(n):
        np.minimum(out, np.take(g, [i], axis=axis) + (u - i) ** 2, out=out)
    return np.minimum(out, NONE)


def squared_edt(source, border=False):
    """``source``: bool [nz][ny][nx].  -> int32 [nz][ny][nx]: 0 at a source; else the squared distance to the nearest
    source, with ``border`` every lattice point beyond the array being one; FAR where there is none."""
    source = np.asarray(source, bool)
    g = np.where(source, np.int64(0), NONE)
    for axis in (2, 1, 0):
        g = axis_minimum(g, axis)
    if border and source.size:
        # the nearest lattice point beyond the box lies straight across the nearest face
        face = None
        for axis, n in enumerate(source.shape):
            shape = [1, 1, 1]
            shape[axis] = n
            c = np.arange(n, dtype=np.int64).reshape(shape)
            f = np.minimum(c + 1, n - c)
            face = f if face is None else np.minimum(face, f)
        g = np.minimum(g, np.broadcast_to(face ** 2, g.shape))
    return np.where(g >= NONE, FAR, g).astype(np.int32)


def box_and_inside(offset, density, labels, box=None, level=None, selected=None, ignore_zero=False):
    """B and inside() as ``components_twin`` decides them -> (offset, lo, n, inside bool [n_z][n_y][n_x] or None for an
    empty B, dropped zeros)."""
    offset = [int(v) for v in offset]
    shape = [0, 0, 0] if density is None else list(np.shape(density)[::-1])
    lo, n = [], []
    for a in range(3):
        b, e = offset[a], offset[a] + shape[a]
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        lo.append(b)
        n.append(e - b)
    if min(n) <= 0:
        return offset, lo, n, None, 0
    cut = tuple(slice(lo[a] - offset[a], lo[a] - offset[a] + n[a]) for a in (2, 1, 0))
    dropped = 0
    if level is not None:
        with np.errstate(invalid="ignore"):
            inside = np.asarray(density, f32)[cut] >= f32(level)               # a NaN is outside
    else:
        lab = np.zeros(tuple(n[::-1]), np.uint32) if labels is None else np.asarray(labels, np.uint32)[cut]
        inside = np.ones(lab.shape, bool) if selected is None else np.isin(lab, np.asarray(list(selected), np.uint32))
        if ignore_zero:
            dropped = int((inside & (lab == 0)).sum())
            inside &= lab != 0
    return offset, lo, n, inside, dropped


def distance_twin(offset, density, labels, box=None, level=None, selected=None, ignore_zero=False, invert=False, border=False):
    """``offset``, ``density``, ``labels``, ``box``, ``level``, ``selected``, ``ignore_zero``: as in ``components_twin``;
    ``invert``, ``border``: svr_distance_params'.  -> dict(header = the 16 words of a call whose capacity is exact, as
    Python ints (negative coordinates as their uint64 patterns), d2 int32 [n_z][n_y][n_x])."""
    offset, lo, n, inside, dropped = box_and_inside(offset, density, labels, box, level, selected, ignore_zero)
    u64 = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF
    if inside is None:
        return dict(header=[0, 0, 0, 0, *[u64(v) for v in offset], 0, 0, 0, 0, 0, 0, 0, 0, 0], d2=np.zeros((0, 0, 0), np.int32))
    target = ~inside if invert else inside
    d2 = squared_edt(~target, border=bool(border) and not invert)
    assert not d2[~target].any() and (d2[target] > 0).all()
    finite = target & (d2 != FAR)
    largest = int(d2[finite].max()) if finite.any() else 0
    first = int(np.flatnonzero((finite & (d2 == largest)).reshape(-1))[0]) if finite.any() else 0
    header = [int(target.sum()), int(inside.sum()), inside.size, largest, *[u64(v) for v in offset], *[u64(v) for v in lo], *n, dropped,
              first, int((target & (d2 == FAR)).sum())]
    return dict(header=header, d2=d2)


def count_only(header):
    """The header of the count-only call, and of a call whose capacity is too small, from the full one."""
    return header[:2] + [0, 0] + header[4:14] + [0, 0]
