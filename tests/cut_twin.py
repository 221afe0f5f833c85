"""numpy float32 restatement of the cut planes (include/svr.h, "cut planes": svr_set_cut_planes), in the operation order
stated there, for both modes, and of svr_composite and svr_iso with them.

The predicate is a function of the ray and of the float counter ``iter``, not of the sample's position or value, so it
cannot be slipped into the other twins through their ``lookup`` the way linear_twin.py does: the two definitions are
restated here with the mask (``composite_cut``, ``iso_cut``) on the pieces the other twins share - the ray set-up
(``iso_twin.setup_rays``), the LOD cascade (``iso_twin.lookup``) and, with ``linear=True``, the linear sample
(``linear_twin.linear_sample``).  With no planes they are the uncut twins bit for bit (tests/test_cut.py holds them to
that).  ``iso_cut`` also returns ``cap``: the index of the cutting plane on a cap hit, -1 elsewhere."""
import numpy as np

import iso_twin
import linear_twin
from iso_twin import _dot, _mv, _unit, setup_rays
from slice_twin import DISCARD, HIT, MISS, hsv_to_rgb

f32 = np.float32
MAX_CUT_PLANES = 8


def host_planes(planes, world):
    """The per-call host part: (g [K, 3], h [K], nhat [K, 3]) in f32 for ``planes`` (K x abcd, world space) and the
    row-major ``world`` matrix (m[4c + r] of the header is world[r, c])."""
    P = np.asarray(planes, f32).reshape(-1, 4)
    W = np.asarray(world, f32)
    g = np.zeros((len(P), 3), f32)
    h = np.zeros(len(P), f32)
    nhat = np.zeros((len(P), 3), f32)
    for k, (a, b, c, d) in enumerate(P):
        for j in range(3):
            g[k, j] = (W[0, j] * a + W[1, j] * b) + W[2, j] * c
        h[k] = ((W[0, 3] * a + W[1, 3] * b) + W[2, 3] * c) - d
        ln = np.sqrt((a * a + b * b) + c * c)
        nhat[k] = (a / ln, b / ln, c / ln)
    return g, h, nhat


class RayCut:
    """A_k and B_k of every ray of a set-up ``S`` (iso_twin.setup_rays), and the predicate on them."""

    def __init__(self, S, planes, mode):
        self.all = str(mode).upper() == "ALL"
        assert self.all or str(mode).upper() == "ANY", mode
        self.g, self.h, self.nhat = host_planes(planes, S["world"])
        assert len(self.g) <= MAX_CUT_PLANES
        size = S["size"]
        p0 = [S["start"][a] * size[a] - f32(0.5) for a in range(3)]
        sd = [S["step"][a] * size[a] for a in range(3)]
        self.A = [_dot(list(g), p0) + h for g, h in zip(self.g, self.h)]
        self.B = [_dot(list(g), sd) for g in self.g]

    def __len__(self):
        return len(self.g)

    def behind(self, k, iters, at=None):
        """behind_k(iter) for the rays ``at`` (an index tuple; default all), ``iters`` a scalar or one per ray."""
        A, B = (self.A[k], self.B[k]) if at is None else (self.A[k][at], self.B[k][at])
        return (A + f32(iters) * B if np.isscalar(iters) else A + iters.astype(f32) * B) < f32(0.0)

    def cut(self, iters, at=None):
        if not len(self):
            return np.False_
        behind = [self.behind(k, iters, at) for k in range(len(self))]
        return np.logical_and.reduce(behind) if self.all else np.logical_or.reduce(behind)


def _lookup(linear):
    return linear_twin._iso_lookup if linear else iso_twin.lookup


def composite_cut(rings, matrices, size, material, table, width, height, alpha_cutoff, color_by_label=False,
                  region=None, pick_id=0, cut_planes=(), cut_mode="ANY", linear=False):
    """svr_composite under svr_set_cut_planes(cut_planes, cut_mode); arguments and result as
    ``composite_twin.composite_twin`` (no census)."""
    with np.errstate(all="ignore"):
        return _composite(rings, matrices, size, material, np.asarray(table, f32), width, height, f32(alpha_cutoff),
                          bool(color_by_label), region, pick_id, cut_planes, cut_mode, _lookup(linear))


def _composite(rings, M, size, mat, T, W, H, cutoff, tint, region, pick_id, planes, mode, lookup):
    S = setup_rays(M, size, mat, W, H, region)
    frag, nsteps, start, step, world, pc, size, shape = (S[k] for k in ("frag", "nsteps", "start", "step", "world", "pc", "size", "shape"))
    rc = RayCut(S, planes, mode)

    K = T.shape[0]
    kmax = f32(K - 1)
    clim0, clim1 = f32(mat["clim"][0]), f32(mat["clim"][1])
    colors = np.asarray(mat["colors"], f32)
    R, G, B, A, w_best = (np.zeros(shape, f32) for _ in range(5))
    best = np.full(shape, -1, np.int64)
    first = np.full(shape, -1, np.int64)
    steps = np.zeros(shape, np.uint32)
    alive = frag.copy()
    it = 0
    while True:
        act = alive & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        coord = [start[k][idx] + f32(it) * step[k][idx] for k in range(3)]
        s, lab, lod = lookup(rings, size, coord)
        res = (lod >= 0) & ~rc.cut(it, idx)                 # a cut sample is a sample no LOD holds
        steps[idx] += 1
        idx = tuple(i[res] for i in idx)
        s, lab = s[res], lab[res]
        v = (s - clim0) / (clim1 - clim0)
        xf = np.fmin(np.fmax(v * kmax, f32(0.0)), kmax)
        j = np.minimum(xf.astype(np.int32), K - 2)
        f = xf - j.astype(f32)
        e = [T[j, c] + f * (T[j + 1, c] - T[j, c]) for c in range(4)]
        if tint:
            hs = colors[lab % np.uint32(len(colors))]
            q = hsv_to_rgb(hs[:, 0], hs[:, 1], np.ones(len(lab), f32))
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

    hit = A > 0
    flags = np.where(hit, HIT, np.where(frag, MISS, DISCARD)).astype(np.uint8)
    rgba = np.zeros(shape + (4,), f32)
    depth = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    pick = np.zeros(shape, np.uint64)
    if hit.any():
        h = np.nonzero(hit)
        a = A[h]
        rgba[h] = np.stack([R[h] / a, G[h] / a, B[h] / a, a * f32(mat["opacity"])], axis=-1)
        cf = [start[k][h] + first[h].astype(f32) * step[k][h] for k in range(3)]
        wp = _mv(world, cf[0] - f32(0.5), cf[1] - f32(0.5), cf[2] - f32(0.5), np.ones_like(cf[0]))
        ndc = _mv(pc, wp[0], wp[1], wp[2], wp[3])
        depth[h] = ndc[2] / np.fmax(ndc[3], f32(0.001))
        cb = [start[k][h] + best[h].astype(f32) * step[k][h] for k in range(3)]
        label[h] = iso_twin.lookup(rings, size, cb)[1]          # labels are the nearest sample's under either sampling
        pick[h] = _pick_word(cb, pick_id, len(h[0]))
    return dict(rgba=rgba, depth=depth, label=label, flags=flags, steps=steps, pick=pick, first=first, best=best)


def _pick_word(c, pick_id, n):
    word = np.full(n, min(int(pick_id), 0xFFFFF), np.uint64)
    for k, shift in enumerate((20, 34, 48)):
        fk = (c[k] * f32(16383.0)).astype(np.float64)
        u = np.where(fk > 0, np.minimum(np.floor(np.nan_to_num(fk, nan=0.0)), 16383.0), 0.0).astype(np.uint64)
        word |= u << np.uint64(shift)
    return word


def iso_cut(rings, matrices, size, material, width, height, params=None, region=None, pick_id=0, cut_planes=(),
            cut_mode="ANY", linear=False):
    """svr_iso under svr_set_cut_planes(cut_planes, cut_mode); arguments and result as ``iso_twin.iso_twin``, plus
    ``cap`` (int32: the plane of a cap hit, -1 elsewhere)."""
    p = dict(iso_twin.DEFAULTS)
    p.update(params or {})
    with np.errstate(all="ignore"):
        return _iso(rings, matrices, size, material, width, height, p, region, pick_id, cut_planes, cut_mode,
                    _lookup(linear))


def _iso(rings, M, size, mat, W, H, p, region, pick_id, planes, mode, lookup):
    S = setup_rays(M, size, mat, W, H, region)
    frag, nsteps, start, step, world, pc, size, shape = (S[k] for k in ("frag", "nsteps", "start", "step", "world", "pc", "size", "shape"))
    rc = RayCut(S, planes, mode)
    world_inv = np.asarray(M["world_inv"], f32)
    iso = f32(p["iso_value"])
    refine = int(p["refine"])

    # ---- coarse search: the first sample at or above the level that is not cut
    cand = np.full(shape, -1, np.int64)
    searching = frag.copy()
    it = 0
    while True:
        act = searching & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        coord = [start[k][idx] + f32(it) * step[k][idx] for k in range(3)]
        s, _, lod = lookup(rings, size, coord)
        got = (lod >= 0) & (s >= iso) & ~rc.cut(it, idx)
        at = tuple(i[got] for i in idx)
        cand[at] = it
        searching[at] = False
        it += 1
    hit = cand >= 0
    flags = np.where(hit, HIT, np.where(frag, MISS, DISCARD)).astype(np.uint8)
    steps = np.where(hit, cand + 1, np.where(frag, nsteps, 0)).astype(np.uint32)
    rgba = np.zeros(shape + (4,), f32)
    depth = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    pick = np.zeros(shape, np.uint64)
    normal = np.zeros(shape + (3,), f32)
    iters = np.full(shape, np.nan, f32)
    cap_plane = np.full(shape, -1, np.int32)
    out = dict(rgba=rgba, depth=depth, label=label, flags=flags, steps=steps, pick=pick, normal=normal, iter=iters,
               cap=cap_plane)
    if not hit.any():
        return out
    h = np.nonzero(hit)
    st = [start[k][h] for k in range(3)]
    sp = [step[k][h] for k in range(3)]
    ci = cand[h]

    # ---- refinement, and pred: the point examined immediately before the hit
    iterf = ci.astype(f32)
    pred = (ci - 1).astype(f32)
    if refine > 1:
        open_ = ci > 0
        base = (ci - 1).astype(f32)
        for k in range(1, refine):
            if not open_.any():
                break
            itk = base + f32(k) / f32(refine)
            s, _, lod = lookup(rings, size, [st[a] + itk * sp[a] for a in range(3)])
            got = open_ & (lod >= 0) & (s >= iso) & ~rc.cut(itk, h)
            iterf = np.where(got, itk, iterf)
            open_ &= ~got
            pred = np.where(open_, itk, pred)
    c = [st[a] + iterf * sp[a] for a in range(3)]
    d = [c[a] * size[a] for a in range(3)]
    _, lab, hl = iso_twin.lookup(rings, size, c)                          # label and LOD: the nearest sample's
    assert (hl >= 0).all()

    # ---- caps
    n_caps = np.zeros(len(ci), bool)
    plane = np.full(len(ci), -1, np.int32)
    if len(rc):
        n_caps = (ci > 0) & rc.cut(pred, h)
        for k in reversed(range(len(rc))):                                # the lowest index wins
            sel = ~rc.behind(k, iterf, h) if rc.all else rc.behind(k, pred, h)
            plane = np.where(n_caps & sel, k, plane)
    cap_plane[h] = plane

    # ---- gradient of the uncut field, view vector, shading
    scales = np.array([r["scale"] for r in rings], f32)[hl]
    g = []
    for a in range(3):
        sa = scales[:, a]
        ha = f32(1.0) / sa
        plus = [d[b] + ha if b == a else d[b] for b in range(3)]
        minus = [d[b] - ha if b == a else d[b] for b in range(3)]
        vp, _, lp = lookup(rings, size, data=plus)
        vm, _, lm = lookup(rings, size, data=minus)
        vp = np.where(lp >= 0, vp, f32(0.0))
        vm = np.where(lm >= 0, vm, f32(0.0))
        g.append((vp - vm) * sa)
    m = world_inv
    G = [(m[0, a] * g[0] + m[1, a] * g[1]) + m[2, a] * g[2] for a in range(3)]
    sd = [sp[a] * size[a] for a in range(3)]
    w = [(world[a, 0] * sd[0] + world[a, 1] * sd[1]) + world[a, 2] * sd[2] for a in range(3)]
    zero = [np.zeros_like(w[0])] * 3
    v = _unit([-w[0], -w[1], -w[2]], zero)
    n = _unit([-G[0], -G[1], -G[2]], v)
    if len(rc):
        capped = plane >= 0
        nh = rc.nhat[np.maximum(plane, 0)]                               # [n, 3]
        nc = [nh[:, a] for a in range(3)]
        flip = _dot(nc, v) < f32(0.0)
        nc = [np.where(flip, -nc[a], nc[a]) for a in range(3)]
        n = [np.where(capped, nc[a], n[a]) for a in range(3)]
    if p["light_direction"] is None:
        l = v
    else:
        l = [np.full_like(v[0], f32(p["light_direction"][a])) for a in range(3)]
    hv = _unit([l[a] + v[a] for a in range(3)], zero)
    ndl = np.abs(_dot(n, l))
    spec = np.abs(_dot(n, hv))
    for _ in range(int(p["shininess_log2"])):
        spec = spec * spec
    if p["color_by_label"]:
        colors = np.asarray(mat["colors"], f32)
        hs = colors[lab % np.uint32(len(colors))]
        base = hsv_to_rgb(hs[:, 0], hs[:, 1], np.ones(len(lab), f32))
    else:
        base = [np.full_like(ndl, f32(p["iso_color"][a])) for a in range(3)]
    t = f32(p["ambient"]) + f32(p["diffuse"]) * ndl
    ss = f32(p["specular"]) * spec
    rgb = [np.fmin(np.fmax(base[a] * t + ss, f32(0.0)), f32(1.0)) for a in range(3)]
    rgba[h] = np.stack(rgb + [np.full_like(ndl, f32(mat["opacity"]))], axis=-1)
    normal[h] = np.stack(n, axis=-1)
    iters[h] = iterf
    wp = _mv(world, c[0] - f32(0.5), c[1] - f32(0.5), c[2] - f32(0.5), np.ones_like(c[0]))
    ndc = _mv(pc, wp[0], wp[1], wp[2], wp[3])
    depth[h] = ndc[2] / np.fmax(ndc[3], f32(0.001))
    label[h] = lab
    pick[h] = _pick_word(c, pick_id, len(h[0]))
    return out
