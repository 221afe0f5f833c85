"""numpy float32 restatement of svr_iso (include/svr.h, "iso-surface render mode"), in the operation order stated there,
under either sampling and with or without cut planes: coarse search, linear refinement, caps where a cut opened the
surface, central-difference gradient at the LOD of the hit, inverse-transpose to world space, two-sided Blinn-Phong
with the specular power by repeated squaring.  No empty-space skipping in it: skipping must not change a plane.  The ray
set-up is the march's and the samples come from the LOD cascade (tests/twin_common.py); the cut predicate is
tests/cut_twin.py's.  Vectorised over pixels: every step advances the pixels whose rays are still searching."""
import numpy as np

from cut_twin import RayCut
from twin_common import (_dot, _unit, flags_of, label_rgb, material_of, matrices_of, ndc_depth,  # noqa: F401  (re-exported)
                         pick_word, sample, setup_rays)

f32 = np.float32

DEFAULTS = dict(iso_value=0.5, refine=4, iso_color=(0.8, 0.8, 0.8), color_by_label=False, ambient=0.2, diffuse=0.7,
                specular=0.3, shininess_log2=5, light_direction=None)


def iso_twin(rings, matrices, size, material, width, height, params=None, region=None, pick_id=0, census=False,
             linear=False, cut_planes=(), cut_mode="ANY"):
    """``rings``: oracle.lmip.rings_of(...); ``matrices``: the six row-major mat4 of svr_camera; ``size``:
    volume_dimensions in shader order; ``params``: the svr_iso_params fields that differ from ``DEFAULTS``; ``linear``:
    S(iter) and D(p) are the linear sample (the label and the LOD of the hit stay the nearest sample's);
    ``cut_planes``, ``cut_mode``: as svr_set_cut_planes takes them.  Returns dict(rgba, depth, label, flags, steps,
    pick, normal, iter, cap) for the output pixels of ``region`` (default: the frame); ``iter`` is the refined float
    counter of the hit (diagnostics), ``cap`` the index of the cutting plane on a cap hit (int32, -1 elsewhere),
    ``nan_before`` the number of NaN samples the coarse search passed, ``gradient_finite`` whether a hit's G is finite.
    ``census``: also "census", the number of samples of the coarse search each LOD resolved (int64 [len(rings)]), and
    "hit_lod", the LOD that holds each hit (int32, -1 on non-hits); nothing else changes."""
    p = dict(DEFAULTS)
    p.update(params or {})
    with np.errstate(all="ignore"):
        out = _iso(rings, matrices, size, material, width, height, p, region, pick_id, census, linear, cut_planes,
                   cut_mode)
    if not census:
        out.pop("census"), out.pop("hit_lod")
    return out


def _iso(rings, M, size, mat, W, H, p, region, pick_id, census, linear, planes, mode):
    S = setup_rays(M, size, mat, W, H, region)
    frag, nsteps, start, step, world, pc, size, shape = (S[k] for k in ("frag", "nsteps", "start", "step", "world", "pc", "size", "shape"))
    rc = RayCut(S, planes, mode)
    world_inv = np.asarray(M["world_inv"], f32)
    iso = f32(p["iso_value"])
    refine = int(p["refine"])

    def data(c):
        return [c[a] * size[a] for a in range(3)]

    # ---- coarse search: the first sample at or above the level that is not cut
    cand = np.full(shape, -1, np.int64)
    searching = frag.copy()
    counts = np.zeros(len(rings), np.int64)
    nan_before = np.zeros(shape, np.int64)                 # diagnostics: NaN samples of the coarse search before the hit
    it = 0
    while True:
        act = searching & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        s, _, lod = sample(rings, data([start[k][idx] + f32(it) * step[k][idx] for k in range(3)]), linear=linear)
        if census:
            counts += np.bincount(lod[lod >= 0], minlength=len(rings))
        got = (lod >= 0) & (s >= iso) & ~rc.cut(it, idx)             # NaN >= iso is false: a NaN sample is passed over
        nan_before[idx] += np.isnan(s)
        at = tuple(i[got] for i in idx)
        cand[at] = it
        searching[at] = False
        it += 1
    hit = cand >= 0
    steps = np.where(hit, cand + 1, np.where(frag, nsteps, 0)).astype(np.uint32)
    rgba = np.zeros(shape + (4,), f32)
    depth = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    pick = np.zeros(shape, np.uint64)
    normal = np.zeros(shape + (3,), f32)
    iters = np.full(shape, np.nan, f32)
    cap = np.full(shape, -1, np.int32)
    hit_lod = np.full(shape, -1, np.int32)
    out = dict(rgba=rgba, depth=depth, label=label, flags=flags_of(hit, frag), steps=steps, pick=pick, normal=normal,
               iter=iters, cap=cap, census=counts, hit_lod=hit_lod, nan_before=nan_before,
               gradient_finite=np.ones(shape, bool))
    if not hit.any():
        return out
    h = np.nonzero(hit)
    st = [start[k][h] for k in range(3)]
    sp = [step[k][h] for k in range(3)]
    ci = cand[h]

    # ---- refinement: linear search of the sub-samples before the candidate; pred: the point examined immediately
    # before the hit
    iterf = ci.astype(f32)
    pred = (ci - 1).astype(f32)
    if refine > 1:
        open_ = ci > 0
        base = (ci - 1).astype(f32)
        for k in range(1, refine):
            if not open_.any():
                break
            itk = base + f32(k) / f32(refine)
            s, _, lod = sample(rings, data([st[a] + itk * sp[a] for a in range(3)]), linear=linear)
            got = open_ & (lod >= 0) & (s >= iso) & ~rc.cut(itk, h)
            iterf = np.where(got, itk, iterf)
            open_ &= ~got
            pred = np.where(open_, itk, pred)
    c = [st[a] + iterf * sp[a] for a in range(3)]
    d = data(c)
    _, lab, hl = sample(rings, d)                                         # label and LOD: the nearest sample's
    assert (hl >= 0).all()
    hit_lod[h] = hl

    # ---- gradient of the uncut field: central differences of one voxel of the hit's LOD per axis, then the
    # inverse-transpose
    scales = np.array([r["scale"] for r in rings], f32)[hl]              # [n, 3]
    g = []
    for a in range(3):
        sa = scales[:, a]
        ha = f32(1.0) / sa
        vp, _, lp = sample(rings, [d[b] + ha if b == a else d[b] for b in range(3)], linear=linear)
        vm, _, lm = sample(rings, [d[b] - ha if b == a else d[b] for b in range(3)], linear=linear)
        vp = np.where(lp >= 0, vp, f32(0.0))
        vm = np.where(lm >= 0, vm, f32(0.0))
        g.append((vp - vm) * sa)
    m = world_inv                                                         # row-major here: m[r, c] = column-major m[4c + r]
    G = [(m[0, a] * g[0] + m[1, a] * g[1]) + m[2, a] * g[2] for a in range(3)]
    sd = [sp[a] * size[a] for a in range(3)]
    w = [(world[a, 0] * sd[0] + world[a, 1] * sd[1]) + world[a, 2] * sd[2] for a in range(3)]
    zero = [np.zeros_like(w[0])] * 3
    v = _unit([-w[0], -w[1], -w[2]], zero)
    n = _unit([-G[0], -G[1], -G[2]], v)
    out["gradient_finite"][h] = np.isfinite(G[0]) & np.isfinite(G[1]) & np.isfinite(G[2])

    # ---- caps: a hit whose predecessor was cut takes the cutting plane's normal, turned towards the viewer
    if len(rc):
        capped = (ci > 0) & rc.cut(pred, h)
        plane = np.full(len(ci), -1, np.int32)
        for k in reversed(range(len(rc))):                                # the lowest index wins
            sel = ~rc.behind(k, iterf, h) if rc.all else rc.behind(k, pred, h)
            plane = np.where(capped & sel, k, plane)
        cap[h] = plane
        capped = plane >= 0
        nh = rc.nhat[np.maximum(plane, 0)]                               # [n, 3]
        nc = [nh[:, a] for a in range(3)]
        flip = _dot(nc, v) < f32(0.0)
        nc = [np.where(flip, -nc[a], nc[a]) for a in range(3)]
        n = [np.where(capped, nc[a], n[a]) for a in range(3)]

    # ---- shading and outputs
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
        base = label_rgb(mat, lab, np.ones(len(lab), f32))
    else:
        base = [np.full_like(ndl, f32(p["iso_color"][a])) for a in range(3)]
    t = f32(p["ambient"]) + f32(p["diffuse"]) * ndl
    ss = f32(p["specular"]) * spec
    rgb = [np.fmin(np.fmax(base[a] * t + ss, f32(0.0)), f32(1.0)) for a in range(3)]
    rgba[h] = np.stack(rgb + [np.full_like(ndl, f32(mat["opacity"]))], axis=-1)
    normal[h] = np.stack(n, axis=-1)
    iters[h] = iterf
    depth[h] = ndc_depth(world, pc, c)
    label[h] = lab
    pick[h] = pick_word(c, pick_id)
    return out


def params_of(material):
    """The ``params`` of ``iso_twin`` for a SubVolumeMaterial in "iso" mode."""
    return dict(iso_value=material.iso_value, refine=material.iso_refine, iso_color=material.iso_color,
                color_by_label=material.color_by_label, ambient=material.ambient, diffuse=material.diffuse,
                specular=material.specular, shininess_log2=material.shininess_log2,
                light_direction=material.light_direction)
