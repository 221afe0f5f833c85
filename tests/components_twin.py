"""numpy restatement of svr_components (include/svr.h): connected components of the box B of one LOD's resident window,
numbered by their first voxels in (z, y, x) order, with the dense volume of numbers, one record per component and the
header.  ``label_components`` works on the box alone (arrays [z][y][x]): the smallest dense index of a component is
spread over shifted views, with pointer jumping, until nothing changes, and the indices that remain are ranked.
``components_twin`` cuts the box out of a window, decides inside() and adds records and header.  No scipy in here: the
CPU test holds this file to ``scipy.ndimage.label``."""
import numpy as np

f32 = np.float32
RECORD = np.dtype([("id", "<u4"), ("label", "<u4"), ("voxels", "<u8"), ("sum", "<u8", 3), ("first", "<i4", 3), ("lo", "<i4", 3),
                   ("hi", "<i4", 3), ("reserved", "<u4")])
assert RECORD.itemsize == 80


def neighbour_offsets(connectivity):
    """The offsets (dz, dy, dx) of a voxel's neighbours: 6 (one axis differs by one) or 26 (any but the voxel itself)."""
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    every = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]
    return every if connectivity == 26 else [d for d in every if sum(abs(v) for v in d) == 1]


def _views(shape, d):
    """(slices of the voxels p that have p + d in the array, slices of those p + d)."""
    here, there = [], []
    for n, v in zip(shape, d):
        here.append(slice(max(0, -v), n - max(0, v)))
        there.append(slice(max(0, v), n - max(0, -v)))
    return tuple(here), tuple(there)


def label_components(inside, key=None, connectivity=6):
    """``inside``: bool [nz][ny][nx]; ``key`` (the same shape, or None): neighbours connect only where their keys are
    equal.  -> (ids u32 [nz][ny][nx], 0 outside and else 1 .. N; roots i64 [N]: the dense index (z n_y + y) n_x + x of
    every component's first voxel, ascending, so that component k + 1 starts at roots[k])."""
    inside = np.asarray(inside, bool)
    shape, n = inside.shape, inside.size
    if n == 0 or not inside.any():
        return np.zeros(shape, np.uint32), np.zeros(0, np.int64)
    if key is not None:
        key = np.asarray(key)
    lab = np.where(inside, np.arange(n, dtype=np.int64).reshape(shape), n)       # n: outside, larger than every index
    pairs = []
    for d in neighbour_offsets(connectivity):
        here, there = _views(shape, d)
        link = inside[here] & inside[there]
        if key is not None:
            link &= key[here] == key[there]
        if link.any():
            pairs.append((here, there, link))
    flat_in = inside.reshape(-1)
    while True:
        new = lab.copy()
        for here, there, link in pairs:
            np.minimum(new[here], np.where(link, lab[there], n), out=new[here])
        flat = new.reshape(-1)
        while True:                                                             # pointer jumping: a label is the index of a voxel of the component
            jumped = np.where(flat_in, flat[np.minimum(flat, n - 1)], n)
            if np.array_equal(jumped, flat):
                break
            flat = jumped
        new = flat.reshape(shape)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[inside])
    ids = np.zeros(shape, np.uint32)
    ids[inside] = (np.searchsorted(roots, lab[inside]) + 1).astype(np.uint32)
    return ids, roots.astype(np.int64)


def components_twin(offset, density, labels, box=None, level=None, selected=None, ignore_zero=False, join_labels=False, connectivity=6):
    """``offset``: the window offset (x, y, z); ``density`` f32 and ``labels`` u32 (None: no label rings): the window
    [z][y][x], None for a window of None; ``box``: (offset, shape) in the LOD's logical voxels (x, y, z) or None;
    ``level``: SVR_COMPONENTS_LEVEL, else SVR_COMPONENTS_LABELS with ``selected`` (ids, or None for every label),
    ``ignore_zero`` and ``join_labels``.  -> dict(header = the 16 words of a call whose capacities are exact, as Python
    ints (negative coordinates as their uint64 patterns), ids u32 [n_z][n_y][n_x], records RECORD [N])."""
    offset = [int(v) for v in offset]
    shape = [0, 0, 0] if density is None else list(np.shape(density)[::-1])
    lo, n = [], []
    for a in range(3):
        b, e = offset[a], offset[a] + shape[a]
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        lo.append(b)
        n.append(e - b)
    u64 = lambda v: int(v) & 0xFFFFFFFFFFFFFFFF
    if min(n) <= 0:
        return dict(header=[0, 0, 0, 0, *[u64(v) for v in offset], 0, 0, 0, 0, 0, 0, 0, 0, 0], ids=np.zeros((0, 0, 0), np.uint32),
                    records=np.zeros(0, RECORD))
    cut = tuple(slice(lo[a] - offset[a], lo[a] - offset[a] + n[a]) for a in (2, 1, 0))
    dropped = 0
    if level is not None:
        with np.errstate(invalid="ignore"):
            inside = np.asarray(density, f32)[cut] >= f32(level)               # a NaN is outside
        lab = np.zeros(inside.shape, np.uint32)
        key = None
    else:
        lab = np.zeros(tuple(n[::-1]), np.uint32) if labels is None else np.asarray(labels, np.uint32)[cut]
        inside = np.ones(lab.shape, bool) if selected is None else np.isin(lab, np.asarray(list(selected), np.uint32))
        if ignore_zero:
            dropped = int((inside & (lab == 0)).sum())
            inside &= lab != 0
        key = None if join_labels else lab
    ids, roots = label_components(inside, key, connectivity)
    N = len(roots)
    records = np.zeros(N, RECORD)
    z, y, x = np.nonzero(inside)
    k = ids[z, y, x].astype(np.int64) - 1
    records["id"] = np.arange(1, N + 1)
    records["voxels"] = np.bincount(k, minlength=N)
    rz, ry, rx = np.unravel_index(roots, inside.shape)
    records["label"] = lab[rz, ry, rx]
    for a, (c, r) in enumerate(((x, rx), (y, ry), (z, rz))):
        total = np.zeros(N, np.uint64)
        np.add.at(total, k, (c + (lo[a] - offset[a])).astype(np.uint64))      # relative to the window offset
        records["sum"][:, a] = total
        records["first"][:, a] = r + lo[a]
        cmin, cmax = np.full(N, np.iinfo(np.int64).max), np.full(N, np.iinfo(np.int64).min)
        np.minimum.at(cmin, k, c)
        np.maximum.at(cmax, k, c)
        records["lo"][:, a], records["hi"][:, a] = cmin + lo[a], cmax + lo[a]
    header = [N, int(inside.sum()), inside.size, N, *[u64(v) for v in offset], *[u64(v) for v in lo], *n, dropped, 0, 0]
    return dict(header=header, ids=ids, records=records)
