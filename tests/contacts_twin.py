"""numpy restatement of svr_contacts (include/svr.h): the voxels B of box and window of one ring of the CPU ring
restatement (``oracle.lmip.rings_of``) gathered through the ring's wrap into a dense block with its own indexing, the
faces of B as three shifted comparisons, the ``selected`` filter and the label-0 drop, then one record per unordered
label pair, sorted by (label_lo, label_hi).  Also a plain triple loop, and ``ContactTable``'s host arithmetic restated
with plain Python numbers."""
import math

import numpy as np

RECORD = np.dtype([("label_lo", "<u4"), ("label_hi", "<u4"), ("faces", "<u8", 3), ("sum2", "<u8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3),
                   ("finite", "<u8"), ("value_sum", "<u8"), ("vmin", "<f4"), ("vmax", "<f4"), ("reserved", "<u8")])
assert RECORD.itemsize == 112


def box_block(ring, box=None):
    """(first voxel (x, y, z), labels [nz][ny][nx] u32, values [nz][ny][nx]) of B: box and window intersected, each
    logical voxel read from slot (x % ring_x, y % ring_y, z % ring_z).  ``box``: (offset, shape) in the LOD's logical
    voxels, shader order; None: the whole window.  An empty B has a zero extent."""
    spans = []
    for a in range(3):
        b, e = int(ring["offset"][a]), int(ring["offset"][a]) + int(ring["shape"][a])
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        spans.append(np.arange(b, max(e, b), dtype=np.int64))
    density = np.asarray(ring["density"])                              # [z][y][x]
    rz, ry, rx = density.shape
    at = np.ix_(spans[2] % rz, spans[1] % ry, spans[0] % rx)
    values = density[at]
    lab = ring.get("labels")
    labels = np.zeros(values.shape, np.uint32) if lab is None else np.asarray(lab)[at].astype(np.uint32)
    first = tuple(int(s[0]) if s.size else 0 for s in spans)
    return first, labels, values


def faces_of(ring, box=None):
    """Every face of B, flat arrays: (axis, lo label, hi label, x, y, z of the owning voxel p, v(p), v(q))."""
    first, labels, values = box_block(ring, box)
    nz, ny, nx = labels.shape
    out = [[] for _ in range(8)]
    if labels.size:
        z, y, x = np.meshgrid(first[2] + np.arange(nz, dtype=np.int64), first[1] + np.arange(ny, dtype=np.int64),
                              first[0] + np.arange(nx, dtype=np.int64), indexing="ij")
        for axis, dim in ((0, 2), (1, 1), (2, 0)):                     # shader axis k is numpy dimension 2 - k
            p = tuple(slice(0, -1) if d == dim else slice(None) for d in range(3))
            q = tuple(slice(1, None) if d == dim else slice(None) for d in range(3))
            lp, lq = labels[p], labels[q]
            face = lp != lq
            cols = (np.full(int(face.sum()), axis, np.int64), np.minimum(lp, lq)[face], np.maximum(lp, lq)[face], x[p][face], y[p][face],
                    z[p][face], values[p][face], values[q][face])
            for o, c in zip(out, cols):
                o.append(c)
    dtypes = (np.int64, np.uint32, np.uint32, np.int64, np.int64, np.int64, values.dtype, values.dtype)
    return tuple(np.concatenate(o) if o else np.zeros(0, dt) for o, dt in zip(out, dtypes)), int(labels.size)


def contacts_twin(ring, box=None, labels=None, ignore_zero=False, integer=None):
    """dict(header = the 8 header words with [0] and [2] of a table that is large enough, records = RECORD array sorted
    by (label_lo, label_hi), abs_sum = per record the f64 sum of the magnitudes of its finite values, integer).
    ``value_sum`` holds the integer sum on integer rings and the bits of a float64 sum on float32 rings.  ``integer``:
    whether the DEVICE ring is u8 / u16 (the CPU restatement keeps those values in float32 arrays); None: by dtype."""
    (axis, lo, hi, x, y, z, vp, vq), voxels = faces_of(ring, box)
    keep = np.ones(lo.shape, bool)
    if labels is not None:
        ids = np.asarray(list(labels), np.uint32)
        keep &= np.isin(lo, ids) | np.isin(hi, ids)
    dropped = 0
    if ignore_zero:
        dropped = int(np.count_nonzero(keep & (lo == 0)))
        keep &= lo != 0
    axis, lo, hi, x, y, z, vp, vq = (c[keep] for c in (axis, lo, hi, x, y, z, vp, vq))
    off = [int(v) for v in ring["offset"]]
    if integer is None:
        integer = np.issubdtype(vp.dtype, np.integer)
    order = np.lexsort((hi, lo))
    axis, lo, hi, x, y, z, vp, vq = (c[order] for c in (axis, lo, hi, x, y, z, vp, vq))
    n = lo.size
    start = np.flatnonzero(np.r_[True, (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])]) if n else np.zeros(0, np.int64)
    rec = np.zeros(start.size, RECORD)
    abs_sum = np.zeros(start.size, np.float64)
    if n:
        rec["label_lo"], rec["label_hi"] = lo[start], hi[start]
        for k, c in enumerate((x, y, z)):
            rec["faces"][:, k] = np.add.reduceat((axis == k).astype(np.uint64), start)
            rec["sum2"][:, k] = np.add.reduceat((2 * (c - off[k]) + (axis == k)).astype(np.uint64), start)
            rec["lo"][:, k] = np.minimum.reduceat(c, start)
            rec["hi"][:, k] = np.maximum.reduceat(c, start)
        # the two values of a face side by side, so that reduceat at 2 * start sums both
        both = np.stack([vp, vq], axis=1).reshape(-1)
        if integer:
            assert np.array_equal(both, both.astype(np.uint64))        # whole numbers, whatever array holds them
            rec["finite"] = 2 * np.add.reduceat(np.ones(n, np.uint64), start)
            rec["value_sum"] = np.add.reduceat(both.astype(np.uint64), 2 * start)
            rec["vmin"] = np.minimum.reduceat(both.astype(np.float32), 2 * start)
            rec["vmax"] = np.maximum.reduceat(both.astype(np.float32), 2 * start)
        else:
            fin = np.isfinite(both)
            wide = np.where(fin, both, 0).astype(np.float64)
            rec["finite"] = np.add.reduceat(fin.astype(np.uint64), 2 * start)
            rec["value_sum"] = np.add.reduceat(wide, 2 * start).view(np.uint64)
            abs_sum = np.add.reduceat(np.abs(wide), 2 * start)
            rec["vmin"] = np.minimum.reduceat(np.where(fin, both, np.inf).astype(np.float32), 2 * start)
            rec["vmax"] = np.maximum.reduceat(np.where(fin, both, -np.inf).astype(np.float32), 2 * start)
    header = [int(start.size), int(n), 0, dropped, off[0], off[1], off[2], voxels]
    return dict(header=header, records=rec, abs_sum=abs_sum, integer=bool(integer))


def brute_force(ring, box=None, labels=None, ignore_zero=False):
    """The same table by a triple loop over the logical voxels, Python numbers only (integer rings) ->
    dict(header, pairs = {(lo, hi): dict of the record's fields})."""
    density, lab = np.asarray(ring["density"]), ring.get("labels")
    rz, ry, rx = density.shape
    off, shape = [int(v) for v in ring["offset"]], [int(v) for v in ring["shape"]]
    b = list(off)
    e = [o + s for o, s in zip(off, shape)]
    if box is not None:
        b = [max(b[a], int(box[0][a])) for a in range(3)]
        e = [min(e[a], int(box[0][a]) + int(box[1][a])) for a in range(3)]
    label = lambda x, y, z: 0 if lab is None else int(lab[z % rz, y % ry, x % rx])
    value = lambda x, y, z: int(density[z % rz, y % ry, x % rx])
    pairs, considered, dropped, voxels = {}, 0, 0, 0
    for z in range(b[2], e[2]):
        for y in range(b[1], e[1]):
            for x in range(b[0], e[0]):
                voxels += 1
                p = (x, y, z)
                for k in range(3):
                    q = tuple(c + (a == k) for a, c in enumerate(p))
                    if q[k] >= e[k] or label(*p) == label(*q):
                        continue
                    lo, hi = sorted((label(*p), label(*q)))
                    if labels is not None and lo not in labels and hi not in labels:
                        continue
                    if ignore_zero and lo == 0:
                        dropped += 1
                        continue
                    considered += 1
                    vs = (value(*p), value(*q))
                    r = pairs.setdefault((lo, hi), dict(faces=[0, 0, 0], sum2=[0, 0, 0], lo=list(p), hi=list(p), finite=0, value_sum=0,
                                                        vmin=vs[0], vmax=vs[0]))
                    r["faces"][k] += 1
                    r["finite"] += 2
                    r["value_sum"] += sum(vs)
                    r["vmin"], r["vmax"] = min(r["vmin"], *vs), max(r["vmax"], *vs)
                    for a, c in enumerate(p):
                        r["sum2"][a] += 2 * (c - off[a]) + (a == k)
                        r["lo"][a], r["hi"][a] = min(r["lo"][a], c), max(r["hi"][a], c)
    return dict(header=[len(pairs), considered, 0, dropped, off[0], off[1], off[2], voxels], pairs=pairs)


def records_of_pairs(pairs):
    """``brute_force``'s pairs as a RECORD array sorted by (label_lo, label_hi)."""
    rec = np.zeros(len(pairs), RECORD)
    for i, key in enumerate(sorted(pairs)):
        r = pairs[key]
        rec[i] = (key[0], key[1], r["faces"], r["sum2"], r["lo"], r["hi"], r["finite"], r["value_sum"], r["vmin"], r["vmax"], 0)
    return rec


# ---- ContactTable's host arithmetic, with plain Python numbers -------------------------------------------------------
def neighbours_twin(records, id):
    """[(partner, area)] of ``id``: the largest area first, ties by the smaller id."""
    rows = []
    for r in records:
        lo, hi = int(r["label_lo"]), int(r["label_hi"])
        if id in (lo, hi):
            rows.append((hi if lo == id else lo, int(r["faces"].sum())))
    return sorted(rows, key=lambda pa: (-pa[1], pa[0]))


def data_area_twin(record, scale):
    """Faces of normal x, y, z times the area of such a face in finest voxels; ``scale``: numpy order (z, y, x)."""
    sx, sy, sz = float(scale[2]), float(scale[1]), float(scale[0])
    fx, fy, fz = (int(v) for v in record["faces"])
    return fz * ((1.0 / sy) * (1.0 / sx)) + fy * ((1.0 / sz) * (1.0 / sx)) + fx * ((1.0 / sz) * (1.0 / sy))


def box_twin(record, scale):
    """``ContactTable.box``: inclusive lo / hi of the owning voxels (shader order), scale in numpy order -> (begin, end)
    of the finest scale in numpy order."""
    begin = tuple(math.floor(float(record["lo"][2 - a]) / float(scale[a])) for a in range(3))
    end = tuple(math.ceil((float(record["hi"][2 - a]) + 1.0) / float(scale[a])) for a in range(3))
    return begin, end


def centroid_twin(record, offset):
    """The mean face centre in LOD voxels, shader order: offset + sum2 / (2 * area)."""
    area = int(record["faces"].sum())
    return tuple(float(offset[a]) + float(int(record["sum2"][a])) / (2.0 * float(area)) for a in range(3))


def position_twin(record, offset, scale, world):
    """``ContactTable.position``: centroid -> finest data coordinate (c + 0.5) / scale - 0.5 -> world (x, y, z)."""
    c = centroid_twin(record, offset)
    data = [(c[a] + 0.5) / float(scale[2 - a]) - 0.5 for a in range(3)] + [1.0]
    return tuple(sum(float(world[r][k]) * data[k] for k in range(4)) for r in range(3))
