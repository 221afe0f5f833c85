"""svr_split (include/svr.h) restated in numpy: the watershed of a dense int32 height field.  Everything is an integer
and fully specified, so the GPU result must equal this one exactly: the header, the dense numbers, every field of every
record.  ``split_brute`` states the same contract a second time as plain loops over voxels, for small boxes: the twin
is held to it in tests/test_split.py."""
import numpy as np

from components_twin import neighbour_offsets

RECORD = np.dtype([("id", "<u4"), ("basins", "<u4"), ("voxels", "<u8"), ("sum", "<u8", 3), ("top", "<i4", 3), ("lo", "<i4", 3),
                   ("hi", "<i4", 3), ("peak", "<i4")])
assert RECORD.itemsize == 80
MAX_MERGE = 1 << 29                    # SVR_SPLIT_MAX_MERGE


def links(a, s, H):
    """Do basins whose lower peak is ``a`` link over a pass of height ``s`` (arrays of int64, or Python ints)?
    t = a - s - H: t <= 0 or t^2 <= 4 H s, in 64-bit integers."""
    t = a - s - H
    return (t <= 0) | (t * t <= 4 * H * s)


def summits_of(height, connectivity):
    """``height`` int32 [nz][ny][nx] -> (inside bool, summit i64 [nz][ny][nx]: the dense index of every inside voxel's
    summit; an outside voxel holds its own index)."""
    height = np.asarray(height, np.int32)
    nz, ny, nx = height.shape
    inside = height > 0
    index = np.arange(height.size, dtype=np.int64).reshape(height.shape)
    # the order as one key: greater height first, then the smaller index; -1 for what can never win
    key = np.where(inside, (height.astype(np.int64) << 32) | (0xFFFFFFFF - index), -1)
    padded = np.full((nz + 2, ny + 2, nx + 2), -1, np.int64)
    padded[1:-1, 1:-1, 1:-1] = key
    best = key.copy()
    for dz, dy, dx in neighbour_offsets(connectivity):
        best = np.maximum(best, padded[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
    up = np.where(inside, 0xFFFFFFFF - (best & 0xFFFFFFFF), index).reshape(-1)
    while True:                                                        # pointer jumping to the fixed point
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    return inside, up.reshape(height.shape)


def split_twin(height, connectivity=26, merge_squared=1):
    """-> dict(header = the 16 words of a call whose capacities are exact, as Python ints; ids u32 [nz][ny][nx];
    records RECORD [N]; and, for the tests of the pieces, summit i64 [nz][ny][nx] (``summits_of``) and seeds i64 [N], the
    seed of every region in id order)."""
    height = np.asarray(height, np.int32)
    if connectivity not in (6, 26) or not 0 <= merge_squared <= MAX_MERGE or min(height.shape) <= 0 or height.size > 1 << 30:
        raise ValueError("svr_split would refuse this")
    nz, ny, nx = height.shape
    H = int(merge_squared)
    inside, summit = summits_of(height, connectivity)
    flat_h = height.reshape(-1).astype(np.int64)
    pairs = []
    for d in neighbour_offsets(connectivity):
        if d > (0, 0, 0):                                              # every unordered pair of neighbours once
            continue
        here = tuple(slice(max(0, -v), n - max(0, v)) for n, v in zip(height.shape, d))
        there = tuple(slice(max(0, v), n - max(0, -v)) for n, v in zip(height.shape, d))
        both = inside[here] & inside[there] & (summit[here] != summit[there])
        sp, sq = summit[here][both], summit[there][both]
        s = np.minimum(height[here][both], height[there][both]).astype(np.int64)
        a = np.minimum(flat_h[sp], flat_h[sq])
        assert (a >= s).all()
        ok = links(a, s, H)
        pairs.append(np.stack([sp[ok], sq[ok]], axis=1))
    pairs = np.unique(np.concatenate(pairs), axis=0) if pairs else np.zeros((0, 2), np.int64)
    # the classes of the links, each named by its smallest summit: a union-find over the few distinct pairs
    summit_list = np.unique(summit[inside])
    parent = {int(s): int(s) for s in summit_list}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for p, q in pairs.tolist():
        p, q = find(p), find(q)
        if p != q:
            parent[max(p, q)] = min(p, q)
    seed_of = np.array([find(int(s)) for s in summit_list], np.int64)
    seeds = np.unique(seed_of)                                          # ascending: region k + 1 has seeds[k]
    N = len(seeds)
    region_of_summit = np.searchsorted(seeds, seed_of) + 1              # per entry of summit_list
    ids = np.zeros(height.shape, np.uint32)
    ids[inside] = region_of_summit[np.searchsorted(summit_list, summit[inside])]

    records = np.zeros(N, RECORD)
    records["id"] = np.arange(1, N + 1)
    records["basins"] = np.bincount(region_of_summit, minlength=N + 1)[1:]
    z, y, x = np.nonzero(inside)
    rid = ids[inside].astype(np.int64)
    records["voxels"] = np.bincount(rid, minlength=N + 1)[1:]
    for ax, c in enumerate((x, y, z)):
        records["sum"][:, ax] = _int_sums(rid, c, N)
        lo = np.full(N + 1, np.iinfo(np.int32).max, np.int64); hi = np.full(N + 1, np.iinfo(np.int32).min, np.int64)
        np.minimum.at(lo, rid, c); np.maximum.at(hi, rid, c)
        records["lo"][:, ax], records["hi"][:, ax] = lo[1:], hi[1:]
    # the top: the summit of the region that beats its others
    skey = (flat_h[summit_list] << 32) | (0xFFFFFFFF - summit_list)
    best = np.full(N + 1, -1, np.int64)
    np.maximum.at(best, region_of_summit, skey)
    top = 0xFFFFFFFF - (best[1:] & 0xFFFFFFFF)
    records["top"] = np.stack([top % nx, top // nx % ny, top // (nx * ny)], axis=1)
    records["peak"] = best[1:] >> 32
    header = [N, int(inside.sum()), height.size, N, len(summit_list)] + [0] * 5 + [nx, ny, nz] + [0] * 3
    return dict(header=header, ids=ids, records=records, summit=summit, seeds=seeds)


def _int_sums(rid, c, N):
    """Exact integer sums of ``c`` per region id 1 .. N."""
    out = np.zeros(N + 1, np.int64)
    np.add.at(out, rid, c.astype(np.int64))
    return out[1:].astype(np.uint64)


def count_only(header):
    """The header of the count-only call from the full one: no ids and no records were written."""
    return header[:2] + [0, 0] + header[4:]


def split_brute(height, connectivity, merge_squared):
    """The contract once more, literally, as loops in pure Python -> (ids as nested lists [z][y][x], records as a list of
    dicts in id order, basins)."""
    nz, ny, nx = len(height), len(height[0]), len(height[0][0])
    offs = neighbour_offsets(connectivity)
    h = lambda i: height[i // (nx * ny)][i // nx % ny][i % nx]
    beats = lambda i, j: h(i) > h(j) or (h(i) == h(j) and i < j)

    def neighbours(i):
        z, y, x = i // (nx * ny), i // nx % ny, i % nx
        for dz, dy, dx in offs:
            if 0 <= z + dz < nz and 0 <= y + dy < ny and 0 <= x + dx < nx:
                yield ((z + dz) * ny + y + dy) * nx + x + dx

    def summit(i):
        while True:
            best = i
            for j in neighbours(i):
                if beats(j, best):
                    best = j
            if best == i:
                return i
            i = best

    inside = [i for i in range(nz * ny * nx) if h(i) > 0]
    S = {i: summit(i) for i in inside}
    group = {s: s for s in set(S.values())}

    def find(v):
        while group[v] != v:
            v = group[v]
        return v

    H = merge_squared
    for p in inside:
        for q in neighbours(p):
            if h(q) > 0 and S[p] != S[q]:
                s, a = min(h(p), h(q)), min(h(S[p]), h(S[q]))
                t = a - s - H
                if t <= 0 or t * t <= 4 * H * s:
                    rp, rq = find(S[p]), find(S[q])
                    if rp != rq:
                        group[max(rp, rq)] = min(rp, rq)
    seeds = sorted({find(s) for s in group})
    number = {seed: k + 1 for k, seed in enumerate(seeds)}
    ids = [[[0] * nx for _ in range(ny)] for _ in range(nz)]
    records = [dict(id=k + 1, basins=0, voxels=0, sum=[0, 0, 0], top=None, lo=[nx, ny, nz], hi=[-1, -1, -1], peak=0) for k in range(len(seeds))]
    for i in inside:
        z, y, x = i // (nx * ny), i // nx % ny, i % nx
        k = number[find(S[i])]
        ids[z][y][x] = k
        r = records[k - 1]
        r["voxels"] += 1
        for ax, c in enumerate((x, y, z)):
            r["sum"][ax] += c; r["lo"][ax] = min(r["lo"][ax], c); r["hi"][ax] = max(r["hi"][ax], c)
    tops = {}
    for s in group:
        k = number[find(s)]
        records[k - 1]["basins"] += 1
        if k not in tops or beats(s, tops[k]):
            tops[k] = s
    for k, s in tops.items():
        records[k - 1]["top"] = [s % nx, s // nx % ny, s // (nx * ny)]
        records[k - 1]["peak"] = h(s)
    return ids, records, len(group)
