"""numpy float32 restatement of svr_composite (include/svr.h, "composite render mode"), in the operation order stated
there.  The ray set-up is the march's (``setup_ray`` in march_kernel.hip), restated here array-at-a-time; ring
contents come from the CPU ring restatement (``oracle.lmip.rings_of``), looked up with the march's LOD cascade.
Vectorised over pixels with an alive mask: every step advances the pixels whose rays are still running."""
import numpy as np

from oracle import lmip
from slice_twin import DISCARD, HIT, MISS, frame_pixels, hsv_to_rgb

f32 = np.float32


def _mv(m, x, y, z, w):
    """M * (x, y, z, w) in the contract's association ((m0 x + m1 y) + m2 z) + m3 w; ``m`` row-major f32."""
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] * w for r in range(4)]


def _mm(a, b):
    out = np.zeros((4, 4), f32)
    for c in range(4):
        col = _mv(a, b[0, c], b[1, c], b[2, c], b[3, c])
        for r in range(4):
            out[r, c] = col[r]
    return out


def material_of(spec_material, colors=None):
    """The uniforms svr_composite reads, from a SceneSpec material dict (defaults of oracle.lmip)."""
    m = dict(lmip.DEFAULT_MATERIAL)
    m.update(spec_material)
    cols = colors if colors is not None else (m["colors"] if m["colors"] is not None else lmip.DEFAULT_COLORS)
    return dict(clim=m["clim"], opacity=m["opacity"], colors=np.array([c[:2] for c in cols], f32),
                clipping_planes=m["clipping_planes"], clipping_mode=m["clipping_mode"])


def lookup(rings, size, coord):
    """The march's sample_vol / sample_segmentations_vol cascade for arrays of normalised coordinates: value, label
    and whether some LOD holds the sample."""
    shape = coord[0].shape
    value = np.zeros(shape, f32)
    label = np.zeros(shape, np.uint32)
    done = np.zeros(shape, bool)
    dd = [coord[k] * size[k] for k in range(3)]
    for r in rings:
        ic = [(dd[k] * f32(r["scale"][k])).astype(np.int32) for k in range(3)]        # trunc, like (int) in the kernel
        inb = np.ones(shape, bool)
        for k in range(3):
            inb &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
        sel = inb & ~done
        if sel.any():
            rz, ry, rx = r["density"].shape
            zi, yi, xi = ic[2][sel] % rz, ic[1][sel] % ry, ic[0][sel] % rx
            value[sel] = np.asarray(r["density"][zi, yi, xi], f32)
            label[sel] = np.asarray(r["labels"][zi, yi, xi]).astype(np.uint32)
        done |= inb
    return value, label, done


def resolving_lod(rings, size, coord=None, data=None):
    """The LOD whose ROI is the first to hold each point (-1: none): the window tests of ``lookup`` alone, which both
    samplings share (the linear sample is taken inside the LOD the nearest sample picks)."""
    dd = [coord[k] * size[k] for k in range(3)] if data is None else data
    lod = np.full(dd[0].shape, -1, np.int32)
    for n, r in enumerate(rings):
        ic = [(dd[k] * f32(r["scale"][k])).astype(np.int32) for k in range(3)]
        inb = lod < 0
        for k in range(3):
            inb &= (r["offset"][k] <= ic[k]) & (ic[k] < r["offset"][k] + r["shape"][k])
        lod[inb] = n
    return lod


def composite_twin(rings, matrices, size, material, table, width, height, alpha_cutoff, color_by_label=False,
                   region=None, pick_id=0, census=False):
    """``rings``: oracle.lmip.rings_of(...); ``matrices``: the six row-major mat4 of svr_camera; ``size``:
    volume_dimensions in shader order; ``table``: the K x 4 f32 device table.  Returns dict(rgba, depth, label, flags,
    steps, pick) for the output pixels of ``region`` (default: the frame).  ``census``: also "census", the number of
    samples each LOD resolved (int64 [len(rings)]); nothing else changes."""
    with np.errstate(all="ignore"):
        return _composite(rings, matrices, size, material, np.asarray(table, f32), width, height, f32(alpha_cutoff),
                          bool(color_by_label), region, pick_id, census)


def _composite(rings, M, size, mat, T, W, H, cutoff, tint, region, pick_id, census=False):
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

    # ---- the samples, front to back
    K = T.shape[0]
    kmax = f32(K - 1)
    clim0, clim1 = f32(mat["clim"][0]), f32(mat["clim"][1])
    colors = np.asarray(mat["colors"], f32)
    shape = x.shape
    R, G, B, A, w_best = (np.zeros(shape, f32) for _ in range(5))
    best = np.full(shape, -1, np.int64)
    first = np.full(shape, -1, np.int64)
    steps = np.zeros(shape, np.uint32)
    alive = frag.copy()
    counts = np.zeros(len(rings), np.int64)
    it = 0
    while True:
        act = alive & (it < nsteps)
        if not act.any():
            break
        idx = np.nonzero(act)
        iterf = f32(it)
        coord = [start[k][idx] + iterf * step[k][idx] for k in range(3)]
        s, lab, res = lookup(rings, size, coord)
        if census:
            held = resolving_lod(rings, size, coord)
            counts += np.bincount(held[held >= 0], minlength=len(rings))
        steps[idx] += 1
        idx = tuple(i[res] for i in idx)                    # samples that no LOD holds contribute nothing
        s, lab = s[res], lab[res]
        v = (s - clim0) / (clim1 - clim0)
        xf = np.fmin(np.fmax(v * kmax, f32(0.0)), kmax)     # NaN -> 0
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

    # ---- outputs
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
        label[h] = lookup(rings, size, cb)[1]
        word = np.full(len(h[0]), min(int(pick_id), 0xFFFFF), np.uint64)
        for k, shift in enumerate((20, 34, 48)):
            fk = (cb[k] * f32(16383.0)).astype(np.float64)
            u = np.where(fk > 0, np.minimum(np.floor(np.nan_to_num(fk, nan=0.0)), 16383.0), 0.0).astype(np.uint64)
            word |= u << np.uint64(shift)
        pick[h] = word
    out = dict(rgba=rgba, depth=depth, label=label, flags=flags, steps=steps, pick=pick)
    if census:
        out["census"] = counts
    return out


def matrices_of(volume, camera):
    """The six row-major mat4 of svr_camera for a SubVolume (its current world transform) and a camera."""
    w = volume.world
    m = {"world": w.matrix, "world_inv": w.inverse_matrix, "cam": camera.view_matrix, "cam_inv": camera.camera_matrix,
         "proj": camera.projection_matrix, "proj_inv": camera.projection_matrix_inverse}
    return {k: np.asarray(v, np.float32) for k, v in m.items()}


def twin_of_spec(spec, table, alpha_cutoff, color_by_label=False, *, matrices=None, region=None, vol=None, rings=None,
                 material=None, pick_id=0):
    """The restatement for a SceneSpec's volume after its ``center_on_position`` calls."""
    vol = vol or lmip.oracle_volume(spec)
    if rings is None:
        rings = lmip.rings_of(vol)
    return composite_twin(rings, matrices if matrices is not None else spec.matrices(), vol.volume_dimensions_shader,
                          material if material is not None else material_of(spec.material), table, spec.width,
                          spec.height, alpha_cutoff, color_by_label, region=region if region is not None else spec.region,
                          pick_id=pick_id)
