"""numpy restatement of svr_objects (include/svr.h): the considered voxels of one LOD's resident window WITH their
logical coordinates (the histogram twin's indexing drops them), the ring wrap, the ``selected`` filter and the label-0
drop taken from the CPU ring restatement (``oracle.lmip.rings_of``), then one record per distinct label.  Also
``ObjectTable.box`` and ``ObjectTable.position`` restated with plain Python numbers."""
import math

import numpy as np

RECORD = np.dtype([("label", "<u4"), ("used", "<u4"), ("voxels", "<u8"), ("sum", "<u8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3),
                   ("finite", "<u8"), ("value_sum", "<u8"), ("vmin", "<f4"), ("vmax", "<f4"), ("reserved", "<u8")])
assert RECORD.itemsize == 96


def considered_voxels(ring, box=None):
    """(x, y, z, label, value), flat arrays, of the voxels of box and window in one ring of ``rings_of``.  ``box``:
    (offset, shape) in the LOD's logical voxels, shader order (x, y, z); None: the whole window.  x, y, z are the
    logical coordinates (int64); the texel comes from slot (x % ring_x, y % ring_y, z % ring_z)."""
    spans = []
    for a in range(3):
        b, e = int(ring["offset"][a]), int(ring["offset"][a]) + int(ring["shape"][a])
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        spans.append(np.arange(b, max(e, b), dtype=np.int64))
    density = np.asarray(ring["density"])                              # [z][y][x]
    rz, ry, rx = density.shape
    zz, yy, xx = np.meshgrid(spans[2], spans[1], spans[0], indexing="ij")
    zz, yy, xx = zz.reshape(-1), yy.reshape(-1), xx.reshape(-1)
    value = density[zz % rz, yy % ry, xx % rx]
    lab = ring.get("labels")
    label = np.zeros(value.shape, np.uint32) if lab is None else np.asarray(lab)[zz % rz, yy % ry, xx % rx].astype(np.uint32)
    return xx, yy, zz, label, value


def objects_twin(ring, box=None, labels=None, ignore_zero=False, integer=None):
    """dict(header = the 8 header words with [0] and [2] of a table that is large enough, objects = {label: dict of the
    record's fields, Python numbers}).  ``value_sum`` is a Python int on integer rings and a float64 ``np.sum`` of the
    finite values on float32 rings, where ``abs_sum`` is the same sum of their magnitudes.  ``integer``: whether the
    DEVICE ring is u8 / u16 (the CPU restatement keeps those values in float32 arrays); None: by the array's dtype."""
    x, y, z, label, value = considered_voxels(ring, box)
    keep = np.ones(label.shape, bool)
    if labels is not None:
        keep &= np.isin(label, np.asarray(list(labels), np.uint32))
    dropped = 0
    if ignore_zero:
        dropped = int(np.count_nonzero(keep & (label == 0)))
        keep &= label != 0
    x, y, z, label, value = x[keep], y[keep], z[keep], label[keep], value[keep]
    off = [int(v) for v in ring["offset"]]
    if integer is None:
        integer = np.issubdtype(value.dtype, np.integer)
    if integer:
        assert np.array_equal(value, value.astype(np.uint64))         # whole numbers, whatever array holds them
        value = value.astype(np.uint64)
    order = np.argsort(label, kind="stable")
    x, y, z, label, value = x[order], y[order], z[order], label[order], value[order]
    ids, first = np.unique(label, return_index=True)
    bounds = list(first) + [label.size]
    objects = {}
    for k, lab in enumerate(ids):
        s = slice(bounds[k], bounds[k + 1])
        xs, ys, zs, vs = x[s], y[s], z[s], value[s]
        rec = dict(voxels=int(xs.size),
                   sum=(int((xs - off[0]).sum()), int((ys - off[1]).sum()), int((zs - off[2]).sum())),
                   lo=(int(xs.min()), int(ys.min()), int(zs.min())), hi=(int(xs.max()), int(ys.max()), int(zs.max())))
        if integer:
            rec.update(finite=int(vs.size), value_sum=int(vs.sum(dtype=np.uint64)), abs_sum=None,
                       vmin=float(np.float32(vs.min())), vmax=float(np.float32(vs.max())))
        else:
            fin = vs[np.isfinite(vs)].astype(np.float64)
            rec.update(finite=int(fin.size), value_sum=float(np.sum(fin)), abs_sum=float(np.sum(np.abs(fin))),
                       vmin=float(np.float32(fin.min())) if fin.size else math.inf,
                       vmax=float(np.float32(fin.max())) if fin.size else -math.inf)
        objects[int(lab)] = rec
    header = [len(objects), int(label.size), 0, dropped, off[0], off[1], off[2], 0]
    return dict(header=header, objects=objects, integer=integer)


def brute_force(ring, box=None, labels=None, ignore_zero=False):
    """The same records by a triple loop over the logical voxels, Python numbers only (integer rings)."""
    density, lab = np.asarray(ring["density"]), ring.get("labels")
    rz, ry, rx = density.shape
    off, shape = [int(v) for v in ring["offset"]], [int(v) for v in ring["shape"]]
    objects, considered, dropped = {}, 0, 0
    for z in range(off[2], off[2] + shape[2]):
        for y in range(off[1], off[1] + shape[1]):
            for x in range(off[0], off[0] + shape[0]):
                if box is not None and not all(box[0][a] <= c < box[0][a] + box[1][a] for a, c in enumerate((x, y, z))):
                    continue
                l = 0 if lab is None else int(lab[z % rz, y % ry, x % rx])
                if labels is not None and l not in labels:
                    continue
                if ignore_zero and l == 0:
                    dropped += 1
                    continue
                considered += 1
                v = int(density[z % rz, y % ry, x % rx])
                r = objects.setdefault(l, dict(voxels=0, sum=[0, 0, 0], lo=[x, y, z], hi=[x, y, z], finite=0, value_sum=0, vmin=v, vmax=v))
                r["voxels"] += 1
                r["finite"] += 1
                r["value_sum"] += v
                r["vmin"], r["vmax"] = min(r["vmin"], v), max(r["vmax"], v)
                for a, c in enumerate((x, y, z)):
                    r["sum"][a] += c - off[a]
                    r["lo"][a], r["hi"][a] = min(r["lo"][a], c), max(r["hi"][a], c)
    return dict(header=[len(objects), considered, 0, dropped, off[0], off[1], off[2], 0], objects=objects)


def box_twin(lo, hi, scale):
    """``ObjectTable.box``: the record's inclusive lo / hi (shader order) and the LOD's scale factor (numpy order) ->
    (begin, end) of the finest scale in numpy order."""
    begin = tuple(math.floor(float(lo[2 - a]) / float(scale[a])) for a in range(3))
    end = tuple(math.ceil((float(hi[2 - a]) + 1.0) / float(scale[a])) for a in range(3))
    return begin, end


def position_twin(rec, offset, scale, world):
    """``ObjectTable.position``: the record's centroid -> finest data coordinate (c + 0.5) / scale - 0.5 -> world (x, y, z).
    ``offset``: header[4..6]; ``scale``: numpy order; ``world``: the 4 x 4 world matrix (rows of Python numbers)."""
    data = []
    for a in range(3):                                                  # shader order
        c = float(offset[a]) + float(rec["sum"][a]) / float(rec["voxels"])
        data.append((c + 0.5) / float(scale[2 - a]) - 0.5)
    data.append(1.0)
    return tuple(sum(float(world[r][k]) * data[k] for k in range(4)) for r in range(3))
