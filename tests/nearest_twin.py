"""numpy restatement of svr_nearest (include/svr.h): the squared distance of every target of the box B of one LOD's
resident window to the nearest source, the dense index of that source and the label there, with the header.  The tie
rule: among the sources at the minimum distance the one with the smallest dense index (z n_y + y) n_x + x wins.

``feature_transform`` works on the box alone: per-axis minima of g[i] + (u - i)^2 in the order x, y, z, each keeping its
FIRST minimiser, composed as z' = oz[z, y, x], y' = oy[z', y, x], x' = ox[z', y', x].  The smallest z among the nearest
sources is the first minimiser along z; within that plane the smallest y, within that row the smallest x: the smallest
dense index.  ``brute_force`` says the rule directly, every target against every source; the CPU test holds the two to
one another.  B and inside() come from ``distance_twin.box_and_inside``.  No scipy in here."""
import numpy as np

from distance_twin import FAR, NONE, box_and_inside


def axis_first_minimum(g, axis):
    """(min over i of g[.., i, ..] + (u - i)^2 along ``axis``, the smallest i that attains it, -1 where nothing does);
    g int64 with NONE for "no source"."""
    n = g.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    u = np.arange(n, dtype=np.int64).reshape(shape)
    out = np.full(g.shape, NONE, np.int64)
    who = np.full(g.shape, -1, np.int64)
    for i in range(n):
        gi = np.take(g, [i], axis=axis)
        cand = np.where(gi >= NONE, NONE, gi + (u - i) ** 2)
        better = cand < out                                             # strictly: an earlier i keeps a tie
        out = np.where(better, cand, out)
        who = np.where(better, i, who)
    return out, who


def feature_transform(source):
    """``source``: bool [nz][ny][nx] -> (d2 int32, FAR where there is no source; index int32, -1 there)."""
    source = np.asarray(source, bool)
    g = np.where(source, np.int64(0), NONE)
    g, ox = axis_first_minimum(g, 2)
    g, oy = axis_first_minimum(g, 1)
    g, oz = axis_first_minimum(g, 0)
    nz, ny, nx = source.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    none = oz < 0
    zz = np.where(none, 0, oz)
    yy = oy[zz, y, x]
    xx = ox[zz, np.where(none, 0, yy), x]
    index = np.where(none, -1, (zz * ny + yy) * nx + xx)
    return np.where(g >= NONE, FAR, g).astype(np.int32), index.astype(np.int32)


def brute_force(source):
    """The definition, every voxel against every source: the minimum squared distance, then the smallest dense index
    among the sources that attain it.  -> (d2 int32, index int32), as ``feature_transform``."""
    source = np.asarray(source, bool)
    nz, ny, nx = source.shape
    coords = np.stack(np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    src = np.flatnonzero(source.reshape(-1))                            # ascending dense indices
    if src.size == 0:
        return np.full(source.shape, FAR, np.int32), np.full(source.shape, -1, np.int32)
    d = ((coords[:, None, :] - coords[src][None, :, :]) ** 2).sum(-1)   # [voxel][source]
    first = d.argmin(axis=1)                                            # argmin keeps the first of equals
    return d.min(axis=1).reshape(source.shape).astype(np.int32), src[first].reshape(source.shape).astype(np.int32)


def tied(source):
    """bool [nz][ny][nx]: the targets with two or more nearest sources."""
    source = np.asarray(source, bool)
    coords = np.stack(np.meshgrid(*[np.arange(n) for n in source.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    src = np.flatnonzero(source.reshape(-1))
    if src.size == 0:
        return np.zeros(source.shape, bool)
    d = ((coords[:, None, :] - coords[src][None, :, :]) ** 2).sum(-1)
    return ((d == d.min(axis=1, keepdims=True)).sum(axis=1) >= 2).reshape(source.shape) & ~source


def nearest_twin(offset, density, labels, box=None, level=None, selected=None, ignore_zero=False, invert=False):
    """Arguments as ``distance_twin`` without ``border``.  -> dict(header = the 16 words of a call whose capacity is exact,
    d2 int32, index int32, label uint32, each [n_z][n_y][n_x])."""
    offset, lo, n, inside, dropped = box_and_inside(offset, density, labels, box, level, selected, ignore_zero)
    u64 = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF
    if inside is None:
        empty = (0, 0, 0)
        return dict(header=[0, 0, 0, 0, *[u64(v) for v in offset], 0, 0, 0, 0, 0, 0, 0, 0, 0], d2=np.zeros(empty, np.int32),
                    index=np.zeros(empty, np.int32), label=np.zeros(empty, np.uint32))
    target = ~inside if invert else inside
    d2, index = feature_transform(~target)
    own = np.arange(target.size).reshape(target.shape)
    assert np.array_equal(index[~target], own[~target]) and not d2[~target].any()      # a source is its own nearest source
    finite = target & (d2 != FAR)
    largest = int(d2[finite].max()) if finite.any() else 0
    first = int(np.flatnonzero((finite & (d2 == largest)).reshape(-1))[0]) if finite.any() else 0
    header = [int(target.sum()), int(inside.sum()), inside.size, largest, *[u64(v) for v in offset], *[u64(v) for v in lo], *n, dropped,
              first, int((target & (d2 == FAR)).sum())]
    label = np.zeros(target.shape, np.uint32)
    if labels is not None:
        cut = tuple(slice(lo[a] - offset[a], lo[a] - offset[a] + n[a]) for a in (2, 1, 0))
        lab = np.asarray(labels, np.uint32)[cut].reshape(-1)
        label = np.where(index >= 0, lab[np.maximum(index, 0)], np.uint32(0)).astype(np.uint32)
    return dict(header=header, d2=d2, index=index, label=label)


def expanded(twin, r):
    """``NearestField.expanded(r)`` from the twin's arrays: the label where d2 <= floor(r^2), 0 elsewhere and at FAR."""
    limit = min(int(np.floor(float(r) * float(r))), FAR - 1)
    return np.where(twin["d2"].astype(np.int64) <= limit, twin["label"], np.uint32(0)).astype(np.uint32)
