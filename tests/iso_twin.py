"""numpy float32 restatement of svr_iso (include/svr.h, "iso-surface render mode"), in the operation order stated there:
coarse search, linear refinement, central-difference gradient at the LOD of the hit, inverse-transpose to world space,
two-sided Blinn-Phong with the specular power by repeated squaring.  No empty-space skipping in it: skipping must not
change a plane.  The ray set-up is the march's, the LOD cascade ``composite_twin.lookup``'s (extended by the LOD index).
Vectorised over pixels: every step advances the pixels whose rays are still searching."""
import numpy as np

from composite_twin import _mm, _mv, material_of as _composite_material, matrices_of, resolving_lod  # noqa: F401  (re-exported)
from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, frame_pixels, hsv_to_rgb

f32 = np.float32

DEFAULTS = dict(iso_value=0.5, refine=4, iso_color=(0.8, 0.8, 0.8), color_by_label=False, ambient=0.2, diffuse=0.7,
                specular=0.3, shininess_log2=5, light_direction=None)


def material_of(spec_material, colors=None):
    """The uniforms svr_iso reads from the material: opacity, colors, clipping planes."""
    return _composite_material(spec_material, colors)


def lookup(rings, size, coord=None, data=None):
    """The LOD cascade for arrays of normalised coordinates (``coord``; d = coord * size) or of data points (``data``):
    value, label, the LOD that holds the point (-1: none)."""
    dd = [coord[k] * size[k] for k in range(3)] if data is None else data
    shape = dd[0].shape
    value = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    lod = np.full(shape, -1, np.int32)
    for n, r in enumerate(rings):
        ic = [(dd[k] * f32(r["scale"][k])).astype(np.int32) for k in range(3)]        # trunc, like (int) in the kernel
        inb = np.ones(shape, bool)
        for k in range(3):
            inb &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
        sel = inb & (lod < 0)
        if sel.any():
            rz, ry, rx = r["density"].shape
            zi, yi, xi = ic[2][sel] % rz, ic[1][sel] % ry, ic[0][sel] % rx
            value[sel] = np.asarray(r["density"][zi, yi, xi], f32)
            label[sel] = np.asarray(r["labels"][zi, yi, xi]).astype(np.uint32)
            lod[sel] = n
    return value, label, lod


def setup_rays(M, size, mat, W, H, region):
    """The march's ``setup_ray`` for every output pixel of ``region`` (as tests/composite_twin.py restates it): frag,
    nsteps, start, step, plus the matrices the outputs need."""
    world = np.asarray(M["world"], f32)
    ndc_to_data = _mm(_mm(np.asarray(M["world_inv"], f32), np.asarray(M["cam_inv"], f32)), np.asarray(M["proj_inv"], f32))
    pc = _mm(np.asarray(M["proj"], f32), np.asarray(M["cam"], f32))
    size = [f32(v) for v in size]
    rel = f32(min(max(np.sqrt(f32(max(size))) / f32(20.0), f32(0.1)), f32(0.8)))

    # ---- setup_ray, per output pixel
    x, y = frame_pixels(W, H, region)
    frag = (x < W) & (y < H)
    px = (f32(2.0) * (x.astype(f32) + f32(0.5))) / f32(W) - f32(1.0)
    py = f32(1.0) - (f32(2.0) * (y.astype(f32) + f32(0.5))) / f32(H)
    one = np.ones_like(px)
    n4 = _mv(ndc_to_data, px, py, -one, one)
    f4 = _mv(ndc_to_data, px, py, one, one)
    far = [f4[k] / f4[3] for k in range(3)]
    near = [n4[k] / n4[3] for k in range(3)]
    d = [far[k] - near[k] for k in range(3)]
    ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ray = [d[k] / ln for k in range(3)]
    t1 = [(f32(-0.5) - near[k]) / ray[k] for k in range(3)]
    t2 = [((size[k] - f32(0.5)) - near[k]) / ray[k] for k in range(3)]
    tmax = [np.fmax(t1[k], t2[k]) for k in range(3)]
    tmin = [np.fmin(t1[k], t2[k]) for k in range(3)]
    t_exit = np.fmin(np.fmin(tmax[0], tmax[1]), tmax[2])
    t_enter = np.fmax(np.fmax(tmin[0], tmin[1]), tmin[2])
    frag &= t_enter <= t_exit
    back = [near[k] + ray[k] * t_exit for k in range(3)]
    bw = _mv(world, back[0], back[1], back[2], one)
    bc = _mv(pc, bw[0], bw[1], bw[2], bw[3])
    frag &= (bc[3] > 0) & (bc[2] >= 0) & (bc[2] <= bc[3])
    planes = np.array(mat.get("clipping_planes", ()), f32).reshape(-1, 4)
    if len(planes):
        behind = [((bw[0] * p[0] + bw[1] * p[1]) + bw[2] * p[2]) < p[3] for p in planes]
        if str(mat.get("clipping_mode", "ANY")).upper() == "ALL":
            frag &= ~np.logical_and.reduce(behind)
        else:
            frag &= ~np.logical_or.reduce(behind)
    nb = [near[k] - back[k] for k in range(3)]
    dist = (nb[0] * ray[0] + nb[1] * ray[1]) + nb[2] * ray[2]
    for k in range(3):
        dist = np.fmax(dist, np.fmin((f32(-0.5) - back[k]) / ray[k], (size[k] - f32(0.5) - back[k]) / ray[k]))
    front = [back[k] + ray[k] * dist for k in range(3)]
    nf = -dist / rel + f32(0.5)
    frag &= nf >= 1.0
    nf = np.where(frag, np.fmin(nf, f32(16777216.0)), f32(1.0))
    nsteps = nf.astype(np.int32)
    nstepsf = nsteps.astype(f32)
    start = [(front[k] + f32(0.5)) / size[k] for k in range(3)]
    step = [((back[k] - front[k]) / size[k]) / nstepsf for k in range(3)]
    return dict(frag=frag, nsteps=nsteps, start=start, step=step, world=world, pc=pc, size=size, shape=x.shape)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unit(v, fallback):
    """v / sqrtf(dot(v, v)) per component, ``fallback`` where the length is 0 or not finite."""
    ln = np.sqrt(_dot(v, v))
    ok = (ln > 0) & np.isfinite(ln)
    safe = np.where(ok, ln, f32(1.0))
    return [np.where(ok, v[k] / safe, fallback[k]) for k in range(3)]


def iso_twin(rings, matrices, size, material, width, height, params=None, region=None, pick_id=0, census=False):
    """``rings``: oracle.lmip.rings_of(...); ``matrices``: the six row-major mat4 of svr_camera; ``size``:
    volume_dimensions in shader order; ``params``: the svr_iso_params fields that differ from ``DEFAULTS``.  Returns
    dict(rgba, depth, label, flags, steps, pick, normal, iter) for the output pixels of ``region`` (default: the frame);
    ``iter`` is the refined float counter of the hit (diagnostics).  ``census``: also "census", the number of samples
    of the coarse search each LOD resolved (int64 [len(rings)]), and "hit_lod", the LOD that holds each hit (int32,
    -1 on non-hits); nothing else changes."""
    p = dict(DEFAULTS)
    p.update(params or {})
    with np.errstate(all="ignore"):
        out = _iso(rings, matrices, size, material, width, height, p, region, pick_id, census)
    if not census:
        out.pop("census"), out.pop("hit_lod")
    return out


def _iso(rings, M, size, mat, W, H, p, region, pick_id, census=False):
    S = setup_rays(M, size, mat, W, H, region)
    frag, nsteps, start, step, world, pc, size, shape = (S[k] for k in ("frag", "nsteps", "start", "step", "world", "pc", "size", "shape"))
    world_inv = np.asarray(M["world_inv"], f32)
    iso = f32(p["iso_value"])
    refine = int(p["refine"])

    # ---- coarse search: the first sample at or above the level
    cand = np.full(shape, -1, np.int64)
    searching = frag.copy()
    counts = np.zeros(len(rings), np.int64)
    hit_lod = np.full(shape, -1, np.int32)
    it = 0
    while True:
        act = searching & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        coord = [start[k][idx] + f32(it) * step[k][idx] for k in range(3)]
        s, _, lod = lookup(rings, size, coord)
        if census:
            counts += np.bincount(lod[lod >= 0], minlength=len(rings))
        got = (lod >= 0) & (s >= iso)
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
    if not hit.any():
        return dict(rgba=rgba, depth=depth, label=label, flags=flags, steps=steps, pick=pick, normal=normal, iter=iters,
                    census=counts, hit_lod=hit_lod)
    h = np.nonzero(hit)
    st = [start[k][h] for k in range(3)]
    sp = [step[k][h] for k in range(3)]
    ci = cand[h]

    # ---- refinement: linear search of the sub-samples before the candidate
    iterf = ci.astype(f32)
    if refine > 1:
        open_ = ci > 0
        base = (ci - 1).astype(f32)
        for k in range(1, refine):
            if not open_.any():
                break
            itk = base + f32(k) / f32(refine)
            s, _, lod = lookup(rings, size, [st[a] + itk * sp[a] for a in range(3)])
            got = open_ & (lod >= 0) & (s >= iso)
            iterf = np.where(got, itk, iterf)
            open_ &= ~got
    c = [st[a] + iterf * sp[a] for a in range(3)]
    d = [c[a] * size[a] for a in range(3)]
    _, lab, hl = lookup(rings, size, c)
    assert (hl >= 0).all()
    hit_lod[h] = hl

    # ---- gradient: central differences of one voxel of the hit's LOD per axis, then the inverse-transpose
    scales = np.array([r["scale"] for r in rings], f32)[hl]              # [n, 3]
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
    m = world_inv                                                         # row-major here: m[r, c] = column-major m[4c + r]
    G = [(m[0, a] * g[0] + m[1, a] * g[1]) + m[2, a] * g[2] for a in range(3)]
    sd = [sp[a] * size[a] for a in range(3)]
    w = [(world[a, 0] * sd[0] + world[a, 1] * sd[1]) + world[a, 2] * sd[2] for a in range(3)]
    zero = [np.zeros_like(w[0])] * 3
    v = _unit([-w[0], -w[1], -w[2]], zero)
    n = _unit([-G[0], -G[1], -G[2]], v)
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
    word = np.full(len(h[0]), min(int(pick_id), 0xFFFFF), np.uint64)
    for k, shift in enumerate((20, 34, 48)):
        fk = (c[k] * f32(16383.0)).astype(np.float64)
        u = np.where(fk > 0, np.minimum(np.floor(np.nan_to_num(fk, nan=0.0)), 16383.0), 0.0).astype(np.uint64)
        word |= u << np.uint64(shift)
    pick[h] = word
    return dict(rgba=rgba, depth=depth, label=label, flags=flags, steps=steps, pick=pick, normal=normal, iter=iters,
                census=counts, hit_lod=hit_lod)


def params_of(material):
    """The ``params`` of ``iso_twin`` for a SubVolumeMaterial in "iso" mode."""
    return dict(iso_value=material.iso_value, refine=material.iso_refine, iso_color=material.iso_color,
                color_by_label=material.color_by_label, ambient=material.ambient, diffuse=material.diffuse,
                specular=material.specular, shininess_log2=material.shininess_log2,
                light_direction=material.light_direction)
