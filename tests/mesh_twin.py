"""numpy restatement of svr_mesh (include/svr.h): naive surface nets over the box B of one LOD's resident window, one
vertex per mixed cell, one quad per crossing lattice edge, f32 arithmetic in the header's order, vertices and quads in
the header's order.  ``surface_nets`` works on the box alone (arrays [z][y][x]); ``mesh_twin`` cuts the box out of a
window, decides inside() and adds the header.  ``area_volume`` is the f64 area and divergence-sum volume of a mesh."""
import numpy as np

f32 = np.float32
# the 12 edges of a cell in the order their crossing points are summed: (axis, corner d0, corner d1), a corner being
# (dx, dy, dz).  Axis x, y, z; within an axis by the offsets on the two other axes, the higher axis the major key.
EDGES = []
for _a in range(3):
    _low, _high = [b for b in range(3) if b != _a]
    for _e in range(4):
        _d0 = [0, 0, 0]
        _d0[_low], _d0[_high] = _e & 1, _e >> 1
        _d1 = list(_d0)
        _d1[_a] = 1
        EDGES.append((_a, tuple(_d0), tuple(_d1)))
assert [e[1][1:] for e in EDGES[:4]] == [(0, 0), (1, 0), (0, 1), (1, 1)]          # x-edges: (dy, dz)


def _corner(p, d):
    """The corner d = (dx, dy, dz) of every cell, from an array padded by one voxel on every side."""
    nz, ny, nx = (s - 1 for s in p.shape)
    return p[d[2]:d[2] + nz, d[1]:d[1] + ny, d[0]:d[0] + nx]


def surface_nets(inside, rel0=(0, 0, 0), values=None, level=None):
    """``inside``: bool [nz][ny][nx] over the box; ``rel0``: the box's first voxel minus the window offset (x, y, z);
    ``values`` (f32, the same shape) and ``level``: SVR_MESH_LEVEL, else every t is 0.5.
    -> (vertices f32 [V, 3] (x, y, z), triangles i32 [T, 3])."""
    inside = np.asarray(inside, bool)
    nz, ny, nx = inside.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), bool)                     # every voxel outside the box is outside
    pad[1:-1, 1:-1, 1:-1] = inside
    corner = {d: _corner(pad, d) for d in [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]}
    stack = np.stack(list(corner.values()))
    active = stack.any(axis=0) & ~stack.all(axis=0)                    # [nz + 1][ny + 1][nx + 1]; cell index i is cell lo - 1 + i
    if values is not None:
        vpad = np.zeros(pad.shape, f32)
        vpad[1:-1, 1:-1, 1:-1] = np.asarray(values, f32)
        upad = np.zeros(pad.shape, bool)                               # in the box and finite
        upad[1:-1, 1:-1, 1:-1] = np.isfinite(np.asarray(values, f32))
        level = f32(level)
    total = [np.zeros(active.shape, f32) for _ in range(3)]
    k = np.zeros(active.shape, np.int32)
    for axis, d0, d1 in EDGES:
        cross = corner[d0] != corner[d1]
        t = np.full(active.shape, f32(0.5), f32)
        if values is not None:
            v0, v1 = _corner(vpad, d0), _corner(vpad, d1)
            with np.errstate(all="ignore"):
                r = (level - v0) / (v1 - v0)                           # f32 throughout
            use = _corner(upad, d0) & _corner(upad, d1) & np.isfinite(r)
            with np.errstate(invalid="ignore"):
                t = np.where(use, np.minimum(np.maximum(r, f32(0.0)), f32(1.0)), f32(0.5)).astype(f32)
        for b in range(3):
            pt = t if b == axis else np.full(active.shape, f32(d0[b]), f32)
            total[b] = (total[b] + np.where(cross, pt, f32(0.0))).astype(f32)      # + 0.0 changes nothing: only crossing edges add
        k += cross
    cz, cy, cx = np.nonzero(active)                                    # ascending z, then y, then x
    assert (k[active] >= 3).all() if cz.size else True
    index = np.full(active.shape, -1, np.int64)
    index[cz, cy, cx] = np.arange(cz.size)
    kf = k[cz, cy, cx].astype(f32)
    vertices = np.empty((cz.size, 3), f32)
    for b, c in enumerate((cx, cy, cz)):
        q = (total[b][cz, cy, cx] / kf).astype(f32)
        vertices[:, b] = ((c + (int(rel0[b]) - 1)).astype(f32) + q).astype(f32)

    keys, quads = [], []
    c0 = corner[(0, 0, 0)]                                             # inside(p) for p = the cell's first corner
    for a in range(3):
        ea = tuple(1 if b == a else 0 for b in range(3))
        pz, py, px = np.nonzero(c0 != corner[ea])
        p = np.stack([px, py, pz], axis=1)                             # (x, y, z)
        eb, ec = np.eye(3, dtype=np.int64)[(a + 1) % 3], np.eye(3, dtype=np.int64)[(a + 2) % 3]
        ks = [p - eb - ec, p - ec, p, p - eb]
        vs = []
        for kk in ks:
            assert (kk >= 0).all(), "a cell around a crossing edge is out of the cell range"
            v = index[kk[:, 2], kk[:, 1], kk[:, 0]]
            assert (v >= 0).all(), "a cell around a crossing edge is not active"
            vs.append(v)
        inp = c0[pz, py, px]
        q = np.where(inp[:, None], np.stack([vs[0], vs[1], vs[2], vs[3]], axis=1), np.stack([vs[0], vs[3], vs[2], vs[1]], axis=1))
        quads.append(q)
        keys.append(((pz * active.shape[1] + py) * active.shape[2] + px) * 3 + a)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    quads = quads[np.argsort(keys, kind="stable")]
    triangles = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, triangles


def mesh_twin(offset, density, labels, box=None, selected=None, level=None):
    """``offset``: the window offset (x, y, z); ``density`` f32 and ``labels`` u32 (None: no label rings): the window
    [z][y][x], None for a window of None; ``box``: (offset, shape) in the LOD's logical voxels (x, y, z) or None; exactly
    one of ``selected`` (ids) and ``level``.  -> dict(vertices, triangles, header = the 8 words of a call whose capacities
    are exact, as Python ints)."""
    assert (selected is None) != (level is None)
    offset = [int(v) for v in offset]
    shape = [0, 0, 0] if density is None else list(density.shape[::-1])
    lo, n = [], []
    for a in range(3):
        b, e = offset[a], offset[a] + shape[a]
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        lo.append(b)
        n.append(e - b)
    if min(n) <= 0:
        return dict(vertices=np.zeros((0, 3), f32), triangles=np.zeros((0, 3), np.int32), header=[0, 0, 0, 0, *offset, 0])
    cut = tuple(slice(lo[a] - offset[a], lo[a] - offset[a] + n[a]) for a in (2, 1, 0))
    values = None
    if selected is not None:
        lab = np.zeros(tuple(n[::-1]), np.uint32) if labels is None else np.asarray(labels)[cut]
        inside = np.isin(lab, np.asarray(list(selected), np.uint32))
    else:
        values = np.asarray(density, f32)[cut]
        with np.errstate(invalid="ignore"):
            inside = values >= f32(level)                              # a NaN is outside
    vertices, triangles = surface_nets(inside, [lo[a] - offset[a] for a in range(3)], values, level)
    header = [len(vertices), len(triangles), len(vertices), len(triangles), *offset, int(inside.sum())]
    return dict(vertices=vertices, triangles=triangles, header=header)


def area_volume(vertices, triangles):
    """(area, enclosed volume) of a mesh in f64: half the cross products' lengths, and the divergence sum
    sum(v0 . (v1 x v2)) / 6, positive when the triangles' normals point outward."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cross = np.cross(b - a, c - a)
    return float(0.5 * np.sqrt((cross * cross).sum(axis=1)).sum()), float((a * np.cross(b, c)).sum() / 6.0)
