"""numpy float32 restatement of svr_histogram (include/svr.h): the considered voxels of one LOD's resident window, its
ring wrap and the label filter taken from the CPU ring restatement (``oracle.lmip.rings_of``), and the binning chain
applied operation by operation.  Also the arithmetic of ``SubVolume.auto_clim`` and the box -> LOD mapping, each
restated on its own (loops and plain Python numbers) so that the package's versions are held to something else."""
import math

import numpy as np

from oracle import lmip

f32 = np.float32


def considered_texels(ring, box=None, labels=None):
    """(values as f32, flat) of the voxels svr_histogram considers in one ring of ``rings_of``.  ``box``: (offset,
    shape) in the LOD's logical voxels, shader order (x, y, z); None: the whole window.  ``labels``: ids to keep."""
    spans = []
    for a in range(3):
        b, e = int(ring["offset"][a]), int(ring["offset"][a]) + int(ring["shape"][a])
        if box is not None:
            b, e = max(b, int(box[0][a])), min(e, int(box[0][a]) + int(box[1][a]))
        spans.append(np.arange(b, max(e, b), dtype=np.int64))
    density = np.asarray(ring["density"])                              # [z][y][x]
    rz, ry, rx = density.shape
    idx = np.ix_(spans[2] % rz, spans[1] % ry, spans[0] % rx)
    v = density[idx].astype(f32).reshape(-1)
    if labels is not None:
        lab = ring.get("labels")
        lab = np.zeros(density.shape, np.uint32) if lab is None else np.asarray(lab)
        v = v[np.isin(lab[idx].astype(np.uint32).reshape(-1), np.asarray(list(labels), np.uint32))]
    return v


def bin_values(v, lo, hi, bins):
    """The binning chain on a flat f32 array: dict(counts u64 [K], tail u64 [4], range f32 [2])."""
    v = np.asarray(v, f32).reshape(-1)
    lo, hi, K = f32(lo), f32(hi), int(bins)
    with np.errstate(over="ignore"):
        inv = f32(K) / (hi - lo)                                       # 0 when hi - lo overflows f32
    assert np.isfinite(inv)
    assert lo < hi
    with np.errstate(invalid="ignore"):
        nan = v != v
        under = ~nan & (v < lo)
        over = ~nan & ~under & (v > hi)
    mid = ~(nan | under | over)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (v[mid] - lo) * inv
    # min((int)x, K - 1), written so that no cast is out of range; a NaN x (inf * 0, svr.h) is bin 0
    with np.errstate(invalid="ignore"):
        j = np.where(x >= f32(K), K - 1, np.where(x > 0, x, f32(0)).astype(np.int32)).astype(np.int64)
    counts = np.bincount(j, minlength=K).astype(np.uint64)
    tail = np.array([under.sum(), over.sum(), nan.sum(), v.size], np.uint64)
    real = v[~nan]
    rng = np.array([real.min(), real.max()] if real.size else [np.inf, -np.inf], f32)
    assert int(counts.sum()) + int(tail[:3].sum()) == int(tail[3])
    return dict(counts=counts, tail=tail, range=rng)


def histogram_twin(rings, lod, lo, hi, bins, box=None, labels=None):
    return bin_values(considered_texels(rings[lod], box, labels), lo, hi, bins)


def histogram_of_spec(spec, lod, lo, hi, bins, box=None, labels=None, vol=None):
    vol = vol or lmip.oracle_volume(spec)
    return histogram_twin(lmip.rings_of(vol), lod, lo, hi, bins, box, labels)


def lod_box_twin(begin, end, scale):
    """(offset, shape) in shader order of the finest-scale box [begin, end) (numpy order) in a LOD's voxels."""
    b = [math.floor(float(x) * float(s)) for x, s in zip(begin, scale)]
    e = [math.ceil(float(x) * float(s)) for x, s in zip(end, scale)]
    return tuple(b[::-1]), tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1]))


def edges_twin(lo, hi, bins):
    lo, hi = float(f32(lo)), float(f32(hi))
    return [lo + (hi - lo) * (j / bins) for j in range(bins + 1)]


def auto_clim_twin(counts, edges, percentiles=(0.5, 99.5)):
    """The pair SubVolume.auto_clim returns, walked bin by bin in Python floats (float64)."""
    counts = [float(c) for c in counts]
    total = sum(counts)
    if total == 0:
        raise ValueError("empty histogram")
    t_lo, t_hi = total * percentiles[0] / 100.0, total * percentiles[1] / 100.0
    lower = upper = None
    c = 0.0
    for j, n in enumerate(counts):
        c += n
        if lower is None and c > t_lo:
            lower = (j, float(edges[j]))
        if upper is None and c >= t_hi:
            upper = float(edges[j + 1])
    if lower is None:
        lower = (len(counts) - 1, float(edges[-2]))
    if upper is None:
        upper = float(edges[-1])
    j, lower = lower
    if upper <= lower:              # equal percentiles whose target a cumulative count meets exactly
        upper = lower + (float(edges[j + 1]) - float(edges[j]))
    return lower, upper
