"""numpy float32 restatement of svr_composite (include/svr.h, "composite render mode"), in the operation order stated
there, under either sampling and with or without cut planes.  The ray set-up is the march's and the samples come from
the LOD cascade (tests/twin_common.py); the cut predicate is tests/cut_twin.py's.  Vectorised over pixels with an alive
mask: every step advances the pixels whose rays are still running."""
import numpy as np

from cut_twin import RayCut
from twin_common import (flags_of, label_rgb, material_of, matrices_of, ndc_depth, pick_word,  # noqa: F401  (re-exported)
                         sample, setup_rays)

f32 = np.float32


def composite_twin(rings, matrices, size, material, table, width, height, alpha_cutoff, color_by_label=False,
                   region=None, pick_id=0, census=False, linear=False, cut_planes=(), cut_mode="ANY"):
    """``rings``: oracle.lmip.rings_of(...); ``matrices``: the six row-major mat4 of svr_camera; ``size``:
    volume_dimensions in shader order; ``table``: the K x 4 f32 device table; ``linear``: s of every sample is the
    linear sample (labels stay the nearest sample's); ``cut_planes``, ``cut_mode``: as svr_set_cut_planes takes them.
    Returns dict(rgba, depth, label, flags, steps, pick, first, best) for the output pixels of ``region`` (default: the
    frame); ``first`` and ``best`` are the counters of the depth's and the label's sample, ``saw_nan`` / ``saw_pinf`` / ``saw_below`` the
    pixels with a contributing sample whose v is NaN / +inf / below 0 (diagnostics).  ``census``:
    also "census", the number of samples each LOD resolved (int64 [len(rings)]); nothing else changes."""
    with np.errstate(all="ignore"):
        return _composite(rings, matrices, size, material, np.asarray(table, f32), width, height, f32(alpha_cutoff),
                          bool(color_by_label), region, pick_id, census, linear, cut_planes, cut_mode)


def _composite(rings, M, size, mat, T, W, H, cutoff, tint, region, pick_id, census, linear, planes, mode):
    S = setup_rays(M, size, mat, W, H, region)
    frag, nsteps, start, step, world, pc, size, shape = (S[k] for k in ("frag", "nsteps", "start", "step", "world", "pc", "size", "shape"))
    rc = RayCut(S, planes, mode)

    # ---- the samples, front to back
    K = T.shape[0]
    kmax = f32(K - 1)
    clim0, clim1 = f32(mat["clim"][0]), f32(mat["clim"][1])
    R, G, B, A, w_best = (np.zeros(shape, f32) for _ in range(5))
    best = np.full(shape, -1, np.int64)
    first = np.full(shape, -1, np.int64)
    steps = np.zeros(shape, np.uint32)
    alive = frag.copy()
    counts = np.zeros(len(rings), np.int64)
    saw = {k: np.zeros(shape, bool) for k in ("nan", "pinf", "below")}     # diagnostics: a contributing sample of that class
    it = 0
    while True:
        act = alive & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        s, lab, lod = sample(rings, [(start[k][idx] + f32(it) * step[k][idx]) * size[k] for k in range(3)], linear=linear)
        if census:
            counts += np.bincount(lod[lod >= 0], minlength=len(rings))
        steps[idx] += 1
        res = (lod >= 0) & ~rc.cut(it, idx)                 # a cut sample is a sample no LOD holds: it contributes nothing
        idx = tuple(i[res] for i in idx)
        s, lab = s[res], lab[res]
        v = (s - clim0) / (clim1 - clim0)
        saw["nan"][idx] |= np.isnan(v)
        saw["pinf"][idx] |= v == np.inf
        saw["below"][idx] |= v < 0
        xf = np.fmin(np.fmax(v * kmax, f32(0.0)), kmax)     # NaN -> 0
        j = np.minimum(xf.astype(np.int32), K - 2)
        f = xf - j.astype(f32)
        e = [T[j, c] + f * (T[j + 1, c] - T[j, c]) for c in range(4)]
        if tint:
            q = label_rgb(mat, lab, np.ones(len(lab), f32))
            e[0], e[1], e[2] = e[0] * q[0], e[1] * q[1], e[2] * q[2]
        a = A[idx]
        w = (f32(1.0) - a) * e[3]
        R[idx] = R[idx] + w * e[0]
        G[idx] = G[idx] + w * e[1]
        B[idx] = B[idx] + w * e[2]
        a = a + w
        A[idx] = a
        better = w > w_best[idx]
        w_best[idx] = np.where(better, w, w_best[idx])
        best[idx] = np.where(better, it, best[idx])
        first[idx] = np.where((first[idx] < 0) & (w > 0), it, first[idx])
        stop = a >= cutoff
        alive[tuple(i[stop] for i in idx)] = False
        it += 1

    # ---- outputs
    hit = A > 0
    rgba = np.zeros(shape + (4,), f32)
    depth = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    pick = np.zeros(shape, np.uint64)
    if hit.any():
        h = np.nonzero(hit)
        a = A[h]
        rgba[h] = np.stack([R[h] / a, G[h] / a, B[h] / a, a * f32(mat["opacity"])], axis=-1)
        depth[h] = ndc_depth(world, pc, [start[k][h] + first[h].astype(f32) * step[k][h] for k in range(3)])
        cb = [start[k][h] + best[h].astype(f32) * step[k][h] for k in range(3)]
        label[h] = sample(rings, [cb[k] * size[k] for k in range(3)])[1]
        pick[h] = pick_word(cb, pick_id)
    out = dict(rgba=rgba, depth=depth, label=label, flags=flags_of(hit, frag), steps=steps, pick=pick, first=first,
               best=best, saw_nan=saw["nan"], saw_pinf=saw["pinf"], saw_below=saw["below"])
    if census:
        out["census"] = counts
    return out

