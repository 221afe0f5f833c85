#!/usr/bin/env python3
"""Differential fuzzing of svr_slice, svr_slab, svr_composite and svr_iso against their numpy twins (tests/*_twin.py)
on the scenes of tools/fuzz_parity.py: 1-4 LODs, anisotropic volumes that are no powers of two, random chunk and ring
shapes, u8 / u16 / f32 data, label-less volumes, a second window move that wraps the rings, world scale and translation,
clipping planes, tiles and stripes - plus, from a generator of their own, the parameters of the four entry points:
sampling, the slice plane, the slab's step / samples / mode, the transfer function / cutoff / tint, the iso level /
refinement / light, cut planes, and the micro-block copy policy.  Every pixel of every plane is compared as
tests/test_gpu_linear.py does (flags, labels, lod, steps, pick, the value plane and the slice's depth bit for bit; rgba,
depth and normal within 1e-4), and three identities that need no twin are held on the same scene: iso with skipping ==
without, slices and slabs from the rows == from the micro-block copy, a MAX slab of one sample == the slice.
usage: fuzz_modes.py [cases] [first_seed] [ortho] [jobs=N]
(prints one line per failing case and entry point, then a summary; jobs=N computes the twins in N CPU processes ahead
of the device, which alone touches the GPU)"""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import fuzz_parity  # noqa: E402
from oracle import lmip  # noqa: E402
from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial, TransferFunction  # noqa: E402

MODE_STREAM = 0x6D6F6465                      # the second word of the mode parameters' seed ("mode")
ENTRY_POINTS = ("slice", "slab", "composite", "iso")
HIT = 2
# The seeds tests/test_gpu_mode_fuzz.py replays, in blocks of ten: 120 perspective cases, then 40 orthographic ones.
# tests/test_mode_fuzz.py holds the census of exactly these on the CPU.  The first seed is a record: keep it.
SUITE_FIRST_SEED = 7064
SUITE_BLOCK = 10
SUITE_BLOCKS = [(SUITE_FIRST_SEED + SUITE_BLOCK * b, False) for b in range(12)] + \
               [(SUITE_FIRST_SEED + SUITE_BLOCK * b, True) for b in range(4)]


def _dot(a, b):
    """Three products summed in order (no BLAS: a seed's digest must not depend on the machine's kernels)."""
    return float(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def _unit(v):
    return v / np.sqrt(_dot(v, v))


def _floats(v):
    return tuple(float(c) for c in v)


RGB_BOUND = 16.0                              # the largest colour value a case may shade (see bounded_clim)


def bounded_clim(spec):
    """The spec's clim, with its upper limit raised where the volume's largest value would shade to a colour above
    RGB_BOUND.  The drawn clim may end far below the data (LODs of mixed types keep bytes against a clim of 0 .. 1), and
    slices and slabs then shade pow(pow(s, gamma), 2.4) of s in the hundreds: colours of 1e5 .. 1e15, whose float32
    spacing alone exceeds the 1e-4 the rgba plane is held to, while the two sides' powf differ by an ulp or a few
    ("Operation-order contract").  With powf good to 16 ulp on either side the chain's relative error is at
    most (2.4 + 1) * 16 * 2^-24 = 3.2e-6, so colours up to 31 stay within 1e-4; 16 leaves a margin.  Values above
    clim[1] stay in the draw (s > 1), only their size is bounded."""
    lo, hi = (float(c) for c in spec.material["clim"])
    top = max(float(np.max(d)) for d, _ in spec.pairs)
    t = RGB_BOUND ** (1.0 / 2.4) * 1.055 - 0.055 if spec.colorspace == "srgb" else RGB_BOUND
    need = lo + (top - lo) / t ** (1.0 / float(spec.material["gamma"]))
    return (lo, max(hi, need))


def random_case(seed, ortho=False):
    """The case ``seed`` names: the scene of ``fuzz_parity.random_spec(seed, ortho=ortho)`` as it is (spec, region,
    variant; of the variant only bits 8 / 9, the routing of slices and slabs, are kept) and the mode parameters, all
    drawn from ``default_rng([seed, MODE_STREAM])``: a new parameter never moves the scene, and new kinds of parameter
    are drawn after the existing ones, behind new arguments.  One field of the scene is narrowed: ``bounded_clim``.  Returns a dict: spec, region, variant, interpolation,
    slice (origin, u, v), slab (w, samples, mode), composite (table, alpha_cutoff, color_by_label), iso (the material's
    iso settings) and cut (planes, mode)."""
    spec, region, variant = fuzz_parity.random_spec(seed, ortho=ortho)
    rng = np.random.default_rng([seed, MODE_STREAM])
    spec.blocked_twin = ("auto", "all", False)[int(rng.integers(0, 3))]
    spec.material["clim"] = bounded_clim(spec)
    interpolation = "linear" if rng.random() < 0.5 else "nearest"
    ws, wp = np.array(spec.world_scale, float), np.array(spec.world_position, float)
    vox = float(ws.mean())                                   # one voxel in world units, as the orthographic draw has it
    data0 = spec.pairs[0][0]
    size_xyz = np.array(data0.shape[::-1], float)

    # ---- the slice: near the last window centre
    centre = np.array(spec.centers[-1][0], float)            # world space
    kind = rng.random()
    if kind < 0.7:                                           # a sub-voxel offset, up to a few voxels away
        origin = centre + (rng.integers(-3, 4, 3) + rng.uniform(-0.5, 0.5, 3)) * ws
    else:                                                    # exactly on a voxel centre (0.15) or a voxel face
        cell = np.round((centre - wp) / ws) + (0.0 if kind < 0.85 else 0.5)
        origin = cell * ws + wp
    p = float(rng.uniform(0.25, 3.0)) * vox
    orient = int(rng.integers(0, 5))
    a, b = rng.normal(size=3), rng.normal(size=3)
    stretch = rng.uniform(0.6, 1.4, 2)
    if orient < 3:
        _, u, v = SubVolume.axis_slice_plane("xyz"[orient], (0.0, 0.0, 0.0), p)
        u, v = np.array(u), np.array(v)
    else:
        ud = _unit(a)
        vd = _unit(np.cross(ud, b))
        if orient == 3:                                      # oblique, orthonormal
            u, v = p * ud, p * np.cross(vd, ud)
        else:                                                # skewed and of unequal length (never parallel)
            u, v = p * stretch[0] * ud, p * stretch[1] * _unit(np.cross(vd, ud) + 0.4 * ud)
    slice_ = dict(origin=_floats(origin), u=_floats(u), v=_floats(v))

    # ---- the slab: the slice's plane, stacked along its normal or obliquely to it
    normal = _unit(np.cross(u, v))
    step = float(rng.uniform(0.3, 2.0)) * vox
    lean = rng.uniform(-0.6, 0.6, 2)
    w = normal * step if rng.random() < 0.5 else (normal + lean[0] * _unit(u) + lean[1] * _unit(v)) * step
    slab = dict(w=_floats(w), samples=int(rng.choice([1, 2, 3, 8, 17, 64])), mode=("max", "min", "mean")[int(rng.integers(0, 3))])

    # ---- the composite mode's table, over the normalised value
    K = int(rng.choice([2, 3, 17, 256, 4096]))
    x = np.linspace(0.0, 1.0, K)
    table = np.empty((K, 4), np.float64)
    table[:, :3] = rng.random((K, 3))
    shape = ("ramp", "step", "spikes", "zero", "opaque")[int(rng.choice(5, p=[0.35, 0.25, 0.15, 0.08, 0.17]))]
    top, at = float(rng.uniform(0.02, 0.9)), float(rng.uniform(0.1, 0.6))
    spikes = rng.integers(0, K, 3)
    if shape == "ramp":
        alpha = top * x
    elif shape == "step":
        alpha = np.where(x >= at, top, 0.0)
    elif shape == "spikes":
        alpha = np.zeros(K)
        for j in spikes:                                     # three spikes, each 1/32 of the range wide (one entry at least)
            alpha[j:j + max(1, K // 32)] = top
    elif shape == "zero":                                    # every ray is a MISS
        alpha = np.zeros(K)
    else:                                                    # opaque from low values: the cutoff stops at the first sample
        alpha = np.where(x >= 0.1 * at, 1.0, 0.0)
    table[:, 3] = alpha
    composite = dict(table=table, alpha_shape=shape, alpha_cutoff=float(rng.choice([1.0, 0.95, 0.5, 1e-3])),
                     color_by_label=bool(rng.random() < 0.5))

    # ---- the iso mode: the level in ring units, from the finest LOD's data
    flat = np.sort(np.asarray(data0, np.float64), axis=None)
    pick = lambda q: float(flat[int(q / 100.0 * (len(flat) - 1))])       # noqa: E731  (a value that occurs in the data)
    kind, q, t = rng.random(), float(rng.uniform(40.0, 90.0)), float(rng.random())
    if kind < 0.75:                                          # between the 40th and the 90th percentile
        level = pick(40.0) + t * (pick(90.0) - pick(40.0))
    elif kind < 0.95:                                        # exactly a value of the data: ties on >=
        level = pick(q)
    else:                                                    # above the maximum: every ray is a MISS
        level = float(flat[-1]) * 1.01 + 1.0
    light = _unit(rng.normal(size=3))
    shade = rng.random(4)
    iso = dict(iso_value=level, iso_refine=int(rng.choice([0, 1, 2, 3, 4, 7, 16])), shininess_log2=int(rng.integers(0, 11)),
               light_direction=None if rng.random() < 0.5 else _floats(light), color_by_label=bool(rng.random() < 0.5),
               ambient=float(shade[0]), diffuse=float(1.5 * shade[1]) if shade[1] > 0.1 else 0.0,
               specular=float(shade[2]) if shade[2] > 0.1 else 0.0, iso_color=_floats(rng.random(3)))

    # ---- cut planes (composite and iso): through points of the volume, as random_spec draws clipping planes
    kind = rng.random()
    count = 0 if kind < 0.4 else int(rng.integers(1, 4)) if kind < 0.82 else 8 if kind < 0.9 else -1
    normals, points = rng.normal(size=(8, 3)), rng.uniform(0.1, 0.9, (8, 3))
    box = np.stack([rng.uniform(0.0, 0.4, 3), rng.uniform(0.6, 1.0, 3)])
    mode = "ALL" if rng.random() < 0.5 else "ANY"
    keep = rng.random() < 0.8                                # under ANY, mostly: the planes face away from the window centre
    if count >= 0:
        planes = []
        for nrm, pt in zip(normals[:count], points[:count]):
            nrm = _unit(nrm)
            d = _dot(nrm, size_xyz * pt * ws + wp)
            if mode == "ANY" and keep and _dot(nrm, centre) < d:  # (a point p is behind a plane where dot(p, abc) < d)
                nrm, d = -nrm, -d
            planes.append(_floats([*nrm, d]))
    else:                                                    # the crop to a random voxel box [begin, end), numpy order
        shape_zyx = np.array(data0.shape)
        begin = np.floor(box[0] * (shape_zyx - 1))
        end = np.maximum(np.ceil(box[1] * shape_zyx), begin + 1)
        planes, mode = SubVolume.crop_planes(types.SimpleNamespace(world=spec.world()), begin, end), "ANY"
    return dict(seed=seed, ortho=bool(ortho), spec=spec, region=region, variant=int(variant) & 0x300,
                interpolation=interpolation, slice=slice_, slab=slab, composite=composite, iso=iso,
                cut=dict(planes=planes, mode=mode, crop=count < 0))


# ---- the settings of a case on a material, and what the twins take ---------------------------------------------------
def apply_composite(material, case):
    c = case["composite"]
    material.render_mode, material.transfer_function = "composite", case.setdefault("_tf", TransferFunction(c["table"]))
    material.alpha_cutoff, material.color_by_label = c["alpha_cutoff"], c["color_by_label"]


def apply_iso(material, case):
    material.render_mode = "iso"
    for k, v in case["iso"].items():
        setattr(material, k, v)


def apply_shared(material, case):
    material.interpolation = case["interpolation"]
    material.cut_planes, material.cut_mode = case["cut"]["planes"], case["cut"]["mode"]


def material_of_case(case):
    """A SubVolumeMaterial as ``testing.build`` makes it from the spec (no device involved)."""
    later = ("clipping_planes", "clipping_mode", "render_mode", "weight_falloff", "cut_planes", "cut_mode")
    spec = case["spec"]
    material = SubVolumeMaterial(**{k: v for k, v in spec.material.items() if k not in later})
    for k in ("clipping_planes", "clipping_mode"):
        if k in spec.material:
            setattr(material, k, spec.material[k])
    return material


def plane_region_fits(region, width, height):
    """svr_slice and svr_slab refuse a region that reaches outside the frame (render_slice's rule); the ray modes
    discard such pixels."""
    if region is None:
        return True
    stripes = 0 < region.band_h < region.out_h
    return not (region.x0 < 0 or region.y0 < 0 or region.out_w < 1 or region.out_h < 1 or region.x0 + region.out_w > width
                or (region.y0 >= height if stripes else region.y0 + region.out_h > height))


def twin_inputs(case, orac=None, matrices=None, world_inv=None, pick_id=0):
    """Everything the four twins read for ``case``, in one dict (the sensitivity tests change one entry of it)."""
    import iso_twin
    import twin_common

    spec = case["spec"]
    orac = orac or lmip.oracle_volume(spec)
    material = material_of_case(case)
    apply_shared(material, case)
    apply_composite(material, case)
    cutoff, tint = material.alpha_cutoff, material.color_by_label
    apply_iso(material, case)
    dims = orac.volume_dimensions_shader
    return dict(rings=lmip.rings_of(orac), dims=dims, matrices=spec.matrices() if matrices is None else matrices,
                world_inv=spec.world().inverse_matrix if world_inv is None else world_inv,
                mat=twin_common.material_of(spec.material), srgb=(spec.colorspace == "srgb"), width=spec.width,
                height=spec.height, region=case["region"], linear=(case["interpolation"] == "linear"),
                plane=dict(case["slice"]), slab=dict(case["slab"]), table=case["_tf"].device_table(dims), cutoff=cutoff,
                tint=tint, iso=iso_twin.params_of(material), tint_iso=material.color_by_label,
                cut_planes=material.cut_planes, cut_mode=material.cut_mode, pick_id=pick_id)


def run_twins(T, which=ENTRY_POINTS):
    """The twins named in ``which`` on the inputs ``T``; slices and slabs only where the region fits the frame."""
    from composite_twin import composite_twin
    from iso_twin import iso_twin
    from slab_twin import slab_twin
    from slice_twin import slice_twin

    W, H, region, out = T["width"], T["height"], T["region"], {}
    pl, fits = T["plane"], plane_region_fits(T["region"], T["width"], T["height"])
    if "slice" in which and fits:
        out["slice"] = slice_twin(T["rings"], T["world_inv"], T["dims"], pl["origin"], pl["u"], pl["v"], W, H, T["mat"],
                                  T["srgb"], region, linear=T["linear"])
    if "slab" in which and fits:
        s = T["slab"]
        out["slab"] = slab_twin(T["rings"], T["world_inv"], T["dims"], pl["origin"], pl["u"], pl["v"], s["w"], s["samples"],
                                s["mode"], W, H, T["mat"], T["srgb"], region, linear=T["linear"])
    cut = dict(linear=T["linear"], cut_planes=T["cut_planes"], cut_mode=T["cut_mode"], region=region, pick_id=T["pick_id"])
    if "composite" in which:
        r = composite_twin(T["rings"], T["matrices"], T["dims"], T["mat"], T["table"], W, H, T["cutoff"], T["tint"], **cut)
        out["composite"] = {k: r[k] for k in ("rgba", "depth", "label", "flags", "steps", "pick")}
    if "iso" in which:
        r = iso_twin(T["rings"], T["matrices"], T["dims"], T["mat"], W, H, T["iso"], **cut)
        out["iso"] = {k: r[k] for k in ("rgba", "depth", "label", "flags", "steps", "pick", "normal")}
    return out


def cpu_side(seed, ortho=False):
    """(case, twins with pick id 0) - everything of a case that needs no device."""
    case = random_case(seed, ortho)
    return case, run_twins(twin_inputs(case))


def hit_counts(refs):
    """HIT pixels per entry point, from the twins' flags (0 where the twin did not run)."""
    return {k: int((refs[k]["flags"] == HIT).sum()) if k in refs else 0 for k in ENTRY_POINTS}


# ---- the comparisons: the mode tests' own ------------------------------------------------------------------------------
SLAB_EXACT, SLAB_CLOSE = ("flags", "label", "lod", "value"), ("rgba", "depth")


def compare(entry, got, ref):
    """``got`` against ``ref`` through the comparison tests/test_gpu_linear.py makes for that entry point; None, or
    (plane, count of bad pixels or maximum error)."""
    import test_gpu_linear as L

    try:
        with contextlib.redirect_stdout(io.StringIO()):
            if entry == "slice":
                L.check_slice(got, ref, entry)
            elif entry == "slab":
                L.check_planes(got, ref, entry, SLAB_EXACT, SLAB_CLOSE)
            else:
                L.check_render(got, ref, entry)
    except AssertionError as e:
        return tuple(e.args[0][1:]) if e.args and isinstance(e.args[0], tuple) else ("?", str(e))
    return None


def same_bits(a, b):
    """None if every plane of ``a`` equals ``b``'s bit for bit, else (plane, differing pixels)."""
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            n = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape else -1
            return (k, n)
    return None


# ---- one case on the device ------------------------------------------------------------------------------------------
def run_case(seed, ortho=False, prepared=None):
    """Build the case's scene once and hold svr_slice, svr_slab, svr_composite and svr_iso to their twins with the drawn
    region, then the identities that need no twin.  Returns (failures, hits): ``failures`` a list of (entry point or
    identity, plane, bad pixels or maximum error), ``hits`` the HIT pixels per entry point from the twins' flags.
    ``prepared``: ``cpu_side(seed, ortho)``, if the caller has it already."""
    import torch

    import twin_common
    from sub_volume_renderer_amd import _native as N, testing
    from test_gpu_iso import host as host_iso
    from test_gpu_slice import host as host_slice

    case, refs = prepared or cpu_side(seed, ortho)
    spec, region, failures = case["spec"], case["region"], []
    W, H = spec.width, spec.height
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    try:
        # the twins ran on the spec's own matrices and pick id 0: the device gets the volume's
        mine, its = spec.matrices(), twin_common.matrices_of(vol, cam)
        assert all(np.array_equal(mine[k], its[k]) for k in its), "the spec's matrices are not the built scene's"
        assert np.array_equal(np.asarray(spec.world().inverse_matrix), np.asarray(vol.world.inverse_matrix))
        for k in ("composite", "iso"):
            hit = refs[k]["flags"] == HIT
            refs[k]["pick"] = np.where(hit, refs[k]["pick"] | np.uint64(min(vol.id, 0xFFFFF)), refs[k]["pick"])

        def held(entry, got, what=None):
            bad = compare(entry, got, refs[entry])
            if bad:
                failures.append((what or entry,) + bad)

        def identical(what, a, b):
            bad = same_bits(a, b)
            if bad:
                failures.append((what,) + bad)

        def variant(v):
            N.check(N.lib().svr_set_variant(vol.prepare(), v), "svr_set_variant")

        def draw_slice():
            r = host_slice(vol.render_slice(*plane, W, H, region=region))
            torch.cuda.synchronize()
            return r

        def draw_slab(samples=None, mode=None):
            s = case["slab"]
            r = host_slice(vol.render_slab(*plane, s["w"], samples or s["samples"], W, H, mode=mode or s["mode"], region=region))
            torch.cuda.synchronize()
            return r

        def draw_render():
            ow, oh = (region.out_w, region.out_h) if region is not None else (W, H)
            out = vol.iso_outputs(ow, oh, count_steps=True, pick=True, normal=(vol.material.render_mode == "iso"))
            vol.render(cam, W, H, region=region, count_steps=True, pick=True, out=out)
            torch.cuda.synchronize()
            return host_iso(out)

        variant(case["variant"])
        apply_shared(vol.material, case)
        pl = case["slice"]
        plane = (pl["origin"], pl["u"], pl["v"])
        if plane_region_fits(region, W, H):
            one = draw_slice()
            held("slice", one)
            held("slab", draw_slab())
            identical("slab(max, 1) == slice", draw_slab(1, "max"), one)
            rows = {}
            for v in (0x100, 0x200):
                variant(v)
                rows[v] = (draw_slice(), draw_slab())
            variant(case["variant"])
            identical("slice rows == copy", *[rows[v][0] for v in rows])
            identical("slab rows == copy", *[rows[v][1] for v in rows])
        else:
            for call in (draw_slice, draw_slab):
                try:
                    call()
                    failures.append((call.__name__, "region", "a region outside the frame was not refused"))
                except ValueError:
                    pass
        apply_composite(vol.material, case)
        held("composite", draw_render())
        apply_iso(vol.material, case)
        skipping = draw_render()
        held("iso", skipping)
        vol.iso_no_skip = True
        identical("iso skip == no_skip", draw_render(), skipping)
        vol.iso_no_skip = False
    finally:
        vol.close()
    return failures, hit_counts(refs)


def _prepare(args):
    try:
        return cpu_side(*args)
    except Exception as e:          # a configuration the reference's own assertions reject
        return e


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    ortho = "ortho" in sys.argv[3:]
    jobs = int(([a.split("=", 1)[1] for a in sys.argv[3:] if a.startswith("jobs=")] or ["1"])[0])
    work = [(seed, ortho) for seed in range(first, first + cases)]
    pool = None
    if jobs > 1:                                             # the twins ahead of the device, in processes that never open it
        import multiprocessing

        pool = multiprocessing.get_context("spawn").Pool(jobs)
        prepared = pool.imap(_prepare, work, chunksize=1)
    else:
        prepared = map(_prepare, work)
    bad = skipped = 0
    with_hits = dict.fromkeys(ENTRY_POINTS, 0)
    try:
        for n, ((seed, _), prep) in enumerate(zip(work, prepared)):
            if n % 100 == 99:                                    # long campaigns: a sign of life
                print(f"... {n + 1} of {cases} cases, {bad} mismatching so far", file=sys.stderr, flush=True)
            if isinstance(prep, Exception):
                skipped += 1
                continue
            try:
                failures, hits = run_case(seed, ortho, prep)     # anything but a mismatch ends the campaign here
            except ValueError as e:                              # the product refused a scene the restatement accepted
                failures, hits = [("refused", type(e).__name__, str(e))], hit_counts({})
            for entry, plane, figure in failures:
                kind = "max error" if isinstance(figure, float) else "bad pixels"
                print(f"seed {seed}{' ortho' if ortho else ''}: MISMATCH {entry}: plane {plane}: {kind} {figure}", flush=True)
            bad += bool(failures)
            for k in ENTRY_POINTS:
                with_hits[k] += hits[k] >= 100
    finally:
        if pool is not None:
            pool.terminate()
    print(f"fuzz_modes{' (orthographic)' if ortho else ''}: {cases} cases from seed {first}: {bad} mismatching, {skipped} "
          f"rejected by the restatement, cases with >= 100 hit pixels: " + ", ".join(f"{k} {v}" for k, v in with_hits.items()),
          flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
