"""GPU: the kernels that draw, on signed and non-finite voxels (tests/special_scenes.py: a signed field with NaN, +-inf,
-0.0, a subnormal and +-3e38 planted as single voxels, macro-cell blocks, a face patch and face-to-face columns).

- The march (`svr_render`): both code objects against the C oracle for LMIP at thresholds +20 / -30 / 0 / +inf, MIP and
  weighted average, from the outside and inside perspective cameras and down an orthographic axis; every kernel
  variant tests/test_gpu_render.py enumerates, each with and without empty-space skipping (variant bit 3), bit for bit
  against the default frame; micro-block copy auto / all / off bit for bit with the census that the copy served
  gathers; step counts bit-exact; and the known answers of the axis views from the voxel columns alone, against the
  device frame directly.
- `svr_slice`, `svr_slab` (max / min / mean, N = 1 / 7 / 16), `svr_composite` and `svr_iso` against their numpy twins,
  nearest and linear, from rows and from the micro-block copy; iso skipping on == off bit for bit with skipped
  stretches counted; slab(max, 1) == slice bit for bit; a cut plane on composite and iso.

Tolerances are those of each mode's own GPU file (integer planes and the value / lod / depth planes of slices and slabs
exact, rgba / depth / normal within 1e-4) under the class rule of tests/helpers.py: a NaN meets any NaN, an infinity
the same infinity, anything else non-finite is an infinite error.  Outputs handed in are pre-filled with sentinels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ortho_scenes as ortho
import special_scenes as S
from helpers import class_error
from oracle import lmip
from slab_twin import twin_of_spec as slab_twin_of
from slice_twin import HIT, MISS, twin_of_spec as slice_twin_of
from sub_volume_renderer_amd import SliceResult, _native as N, testing
from test_gpu_composite import check as check_render, composite_on, host as host_render
from test_gpu_cut import comp_ref, iso_ref
from test_gpu_iso import assert_same_planes, check as check_iso, host as host_iso, iso_on
from test_gpu_linear import check_planes
from test_gpu_slice import host as host_slice

pytestmark = pytest.mark.gpu
TOL = 1e-4
NO_SKIP, ROWS, ALWAYS = 0x008, 0x100, 0x200
VARIANTS = [0x000, 0x200, 0x100, 0x001, 0x250, 0x230, 0x202, 0x2200, 0x4200, 0xE202]      # tests/test_gpu_render.py
MARCH_VIEWS = ("outside", "inside", "+y")
SHADINGS = list(S.SHADING)


def set_variant(vol, variant):
    N.check(N.lib().svr_set_variant(vol.prepare(), variant), "svr_set_variant")


def twin_batches(vol) -> int:
    tm = (C.c_uint64 * 16)()
    N.check(N.lib().svr_debug_timers(vol._rings.handle, tm, 1), "svr_debug_timers")
    return int(tm[15])


def hold(vol, cam, spec, ref):
    """Both code objects against the oracle on every plane, the pick plane included."""
    rep = testing.hold_both_to(ref, vol, cam, spec.width, spec.height, tol=TOL, pick=True)
    for r in (rep["production"], rep["instrumented"]):
        assert np.array_equal(r.pick.cpu().numpy().view(np.uint64), ref.pick)
    return rep


def same_frames(a, b, what, pick_ids_differ=False):
    same = testing.planes_identical(a, b)
    if pick_ids_differ:                                 # two volumes: the low 20 bits of a pick word are the volume's id
        same["pick"] = bool(torch.equal(a.pick.view(torch.int64) >> 20, b.pick.view(torch.int64) >> 20))
    assert same and all(same.values()), (what, same)
    if a.steps is not None and b.steps is not None:
        assert torch.equal(a.steps, b.steps), (what, "steps")


# ---- the march ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(S.MARCH))
@pytest.mark.parametrize("view", MARCH_VIEWS)
def test_march_matches_the_oracle_under_every_variant(view, mode):
    shading = SHADINGS[(list(S.MARCH).index(mode) + MARCH_VIEWS.index(view)) % len(SHADINGS)]
    spec = S.march_spec(view, mode, shading)
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    assert vol._rings.density_storage == "float32"
    ref = lmip.render_spec(spec, pick_id=vol.id)
    rep = hold(vol, cam, spec, ref)
    base_prod, base_inst = rep["production"], rep["instrumented"]
    print(view, mode, shading, "hit", rep["n_hit"], "miss", rep["n_miss"], "rgba max rel", rep["rgba_max_rel"],
          "non-finite rgba pixels", int((~np.isfinite(ref.rgba)).any(-1).sum()))
    assert rep["n_hit"] + rep["n_miss"] > 1000
    for variant in VARIANTS:
        for v in (variant, variant | NO_SKIP):
            set_variant(vol, v)
            prod, inst = testing.render_both(vol, cam, spec.width, spec.height, pick=True)
            same_frames(prod, base_prod, (view, mode, hex(v), "production"))
            same_frames(inst, base_inst, (view, mode, hex(v), "instrumented"))
    set_variant(vol, 0)
    vol.close()


@pytest.mark.parametrize("mode", ["lmip+20", "lmip+inf", "mip", "wavg"])
def test_micro_block_copy_policies_give_the_same_frames(mode):
    frames = {}
    for copy in ("auto", "all", False):
        spec = S.march_spec("outside", mode, "above-g1.6-linear")
        spec.blocked_twin = copy
        scene = testing.build(spec)
        vol = scene.volume
        assert bool(vol._rings.blocked_twin[0]) == (copy is not False)
        ref = lmip.render_spec(spec, pick_id=vol.id)
        for variant in (0, ALWAYS) if copy else (0,):
            set_variant(vol, variant)
            twin_batches(vol)
            rep = hold(vol, scene.camera, spec, ref)
            frames[(copy, variant)] = (rep["production"], rep["instrumented"])
            if variant == ALWAYS:
                served = twin_batches(vol)
                print(mode, copy, "batches gathered from the copy", served)
                assert served > 0
        set_variant(vol, 0)
        vol.close()
    first = frames[("auto", 0)]
    for key, (prod, inst) in frames.items():
        same_frames(prod, first[0], (mode, key), pick_ids_differ=True)
        same_frames(inst, first[1], (mode, key), pick_ids_differ=True)


@pytest.mark.parametrize("view", S.ORTHO_VIEWS)
def test_axis_views_show_what_their_voxel_columns_hold(view):
    """No oracle: MIP is the first argmax of |v| over the column's non-NaN voxels, an LMIP run starts at the first voxel
    with |v| >= threshold and walks on as special_scenes.lmip_walk restates it, a column without such a voxel is a MISS;
    grey, unfogged, linear shading shows (v - clim0) / (clim1 - clim0) itself."""
    grey = dict(colors=[(0.0, 0.0, 1.0)], fog_density=0.0)
    for mode in ("mip", "lmip+20", "lmip-30"):
        spec = S.march_spec(view, mode, "wide-g1-srgb", **grey)
        spec.colorspace = "linear"
        scene = testing.build(spec)
        vol = scene.volume
        orac = lmip.oracle_volume(spec)
        thr = spec.material["lmip_threshold"]
        ka = S.column_answers(spec, orac, "mip" if mode == "mip" else "first", thr)
        J, (iu, iv) = ka["judged"], ka["columns"]
        assert J.sum() == 64 * 64 and (ka["flags"][J] == 1).sum() >= 64
        lo, hi = S.depth_bounds(spec, np.maximum(ka["index"], 0), ka["axis"])
        picked = list(zip(*np.nonzero(J)))[::37]
        for variant in (0, ALWAYS, 0x001):
            set_variant(vol, variant)
            for r in testing.render_both(vol, scene.camera, spec.width, spec.height):
                f = r.flags.cpu().numpy()
                assert np.array_equal(f[J], ka["flags"][J]), (view, mode, variant, int((f[J] != ka["flags"][J]).sum()))
                if mode == "mip":
                    hit = J & (ka["flags"] == 2)
                    want = ((ka["value"][hit] - np.float32(-60.0)) / np.float32(120.0)).astype(np.float32)
                    got = r.rgba.cpu().numpy()
                    for ch in range(3):
                        err = class_error(got[..., ch][hit], want) / np.maximum(1.0, np.abs(np.nan_to_num(want)))
                        assert float(err.max()) <= 2e-6, (view, variant, ch, float(err.max()))
                    assert np.array_equal(r.label_numpy()[hit], ka["label"][hit]), (view, variant)
                    dep = r.depth.cpu().numpy()[hit]
                    assert np.all(dep >= lo[hit] - 1e-6) and np.all(dep <= hi[hit] + 1e-6)
                    print(view, variant, "MIP winners: +inf", int((ka["value"][hit] == np.inf).sum()), "-inf",
                          int((ka["value"][hit] == -np.inf).sum()), "negative", int((ka["value"][hit] < 0).sum()))
                else:
                    lab = r.label_numpy()
                    for j, i in picked:
                        col = ortho.column_of(ka["val_xyz"], ka["axis"], 1.0, iu[j, i], iv[j, i])
                        win, steps = S.lmip_walk(col, thr, 0.5, 10)
                        assert (f[j, i] == 2) == (win >= 0), (view, mode, j, i)
                        if win >= 0:
                            assert lab[j, i] == ortho.column_of(ka["lab_xyz"], ka["axis"], 1.0, iu[j, i], iv[j, i])[win]
                        if r.steps is not None:
                            assert int(r.steps.cpu().numpy().view(np.uint32)[j, i]) == steps, (view, mode, j, i)
        set_variant(vol, 0)
        vol.close()


# ---- slices and slabs -----------------------------------------------------------------------------------------------
def sentinel_slice(w, h):
    dev = torch.device("cuda", torch.cuda.current_device())
    return SliceResult(torch.full((h, w, 4), 7.0, device=dev), torch.full((h, w), 7.0, device=dev),
                       torch.full((h, w), 7, dtype=torch.int32, device=dev), torch.full((h, w), 7, dtype=torch.uint8, device=dev),
                       None, value=torch.full((h, w), 7.0, device=dev), lod=torch.full((h, w), 7, dtype=torch.uint8, device=dev))


@functools.lru_cache(maxsize=None)
def plane_refs(shading, linear):
    """The twins' planes for every slice and slab of one shading, computed once and shared by the routing variants."""
    spec = S.march_spec("outside", "mip", shading)
    orac = lmip.oracle_volume(spec)
    W, H = spec.width, spec.height
    refs = {}
    for name, o, u, v in S.planes():
        refs[("slice", name)] = slice_twin_of(spec, o, u, v, W, H, vol=orac, linear=linear)
        for n in S.SLAB_SAMPLES:
            for mode in S.SLAB_MODES:
                refs[("slab", name, n, mode)] = slab_twin_of(spec, o, u, v, S.SLAB_W[name], n, mode, W, H, vol=orac, linear=linear)
    return refs


@functools.lru_cache(maxsize=None)
def slab_values(shading, name, n):
    spec = S.march_spec("outside", "mip", shading)
    o, u, v = next(p[1:] for p in S.planes() if p[0] == name)
    return S.slab_columns(spec, lmip.oracle_volume(spec), o, u, v, S.SLAB_W[name], n)


@pytest.mark.parametrize("linear", [False, True], ids=["nearest", "linear"])
@pytest.mark.parametrize("shading", ["wide-g1-srgb", "above-g1.6-linear"])
def test_slices_and_slabs_match_the_twins(shading, linear):
    spec = S.march_spec("outside", "mip", shading)
    spec.blocked_twin = "all"
    vol = testing.build(spec).volume
    W, H = spec.width, spec.height
    refs = plane_refs(shading, linear)
    interp = "linear" if linear else "nearest"
    arithmetic_nan_bits = set()                         # (twin bits, device bits) where a mean of +inf and -inf made a NaN
    n_special = 0
    for variant in (0, ROWS, ALWAYS):
        set_variant(vol, variant)
        for name, o, u, v in S.planes():
            out = sentinel_slice(W, H)
            assert vol.render_slice(o, u, v, W, H, interpolation=interp, out=out) is out
            torch.cuda.synchronize()
            sl = {k: a.copy() for k, a in host_slice(out).items()}
            ref = refs[("slice", name)]
            check_planes(sl, ref, ("slice", shading, interp, variant, name), ("flags", "label", "lod", "value", "depth"), ("rgba",))
            n_special += int((~np.isfinite(ref["value"])).sum())
            for n in S.SLAB_SAMPLES:
                for mode in S.SLAB_MODES:
                    out = sentinel_slice(W, H)
                    vol.render_slab(o, u, v, S.SLAB_W[name], n, W, H, mode=mode, interpolation=interp, out=out)
                    torch.cuda.synchronize()
                    got = host_slice(out)
                    ref = refs[("slab", name, n, mode)]
                    # the slab's depth plane: bits in tests/test_gpu_slab.py (nearest), within TOL in test_gpu_linear.py
                    check_planes(got, ref, ("slab", shading, interp, variant, name, n, mode),
                                 ("flags", "label", "lod", "value") + (() if linear else ("depth",)),
                                 ("rgba",) + (("depth",) if linear else ()))
                    if mode == "mean" and not linear:
                        vals, held = slab_values(shading, name, n)
                        made = np.isnan(ref["value"]) & ~(np.isnan(vals) & held).any(0)     # no NaN sample in the column
                        pairs = np.stack([ref["value"].view(np.uint32)[made], got["value"].view(np.uint32)[made]], -1)
                        arithmetic_nan_bits |= {tuple(int(b) for b in p) for p in np.unique(pairs, axis=0)} if made.any() else set()
                    if (n, mode) == (1, "max"):                 # slab(max, 1) == slice on every plane, on the device
                        for k in sl:
                            assert np.array_equal(sl[k].view(np.uint8), got[k].view(np.uint8)), ("N = 1", name, k)
    set_variant(vol, 0)
    print(shading, interp, "non-finite slice values", n_special, "NaNs made by inf + -inf in a mean, (twin, device) bits",
          sorted((hex(a), hex(b)) for a, b in arithmetic_nan_bits))
    assert n_special > 300
    vol.close()


def test_linear_samples_on_voxel_centres_meet_non_finite_corners_at_weight_zero():
    """The centre planes of special_scenes: inside LOD 0 every fraction of the 8-corner blend is exactly 0, so a NaN or
    infinite corner enters as 0 * NaN or 0 * inf.  Slices and slabs (whose unit step keeps the samples on centres),
    from rows and from the micro-block copy, against the twins; the census is tests/test_special_values.py's."""
    spec = S.march_spec("outside", "mip")
    spec.blocked_twin = "all"
    vol = testing.build(spec).volume
    orac = lmip.oracle_volume(spec)
    W, H = spec.width, spec.height
    n_zero_weight = 0
    for name, o, u, v, w in S.centre_planes():
        near = slice_twin_of(spec, o, u, v, W, H, vol=orac)
        ref = slice_twin_of(spec, o, u, v, W, H, vol=orac, linear=True)
        slabs = {(n, mode): slab_twin_of(spec, o, u, v, w, n, mode, W, H, vol=orac, linear=True)
                 for n, mode in ((7, "max"), (7, "min"), (7, "mean"), (1, "max"))}
        n_zero_weight += int(((near["lod"] == 0) & np.isfinite(near["value"]) & np.isnan(ref["value"])).sum())
        for variant in (0, ROWS, ALWAYS):
            set_variant(vol, variant)
            out = sentinel_slice(W, H)
            vol.render_slice(o, u, v, W, H, interpolation="linear", out=out)
            torch.cuda.synchronize()
            check_planes(host_slice(out), ref, ("centre slice", name, variant), ("flags", "label", "lod", "value", "depth"), ("rgba",))
            for (n, mode), sref in slabs.items():
                out = sentinel_slice(W, H)
                vol.render_slab(o, u, v, w, n, W, H, mode=mode, interpolation="linear", out=out)
                torch.cuda.synchronize()
                check_planes(host_slice(out), sref, ("centre slab", name, variant, n, mode), ("flags", "label", "lod", "value"),
                             ("rgba", "depth"))
    set_variant(vol, 0)
    print("finite voxels whose linear sample a weight-0 corner made NaN", n_zero_weight)
    assert n_zero_weight >= 30
    vol.close()


# ---- composite and iso ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", [False, True], ids=["nearest", "linear"])
@pytest.mark.parametrize("view", MARCH_VIEWS)
def test_composite_matches_the_twin(view, linear):
    spec = S.march_spec(view, "mip", "wide-g1-srgb")
    spec.blocked_twin = "all"
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    vol.material.interpolation = "linear" if linear else "nearest"
    n_hit = 0
    for cut in (None, S.CUT):
        vol.material.cut_planes, vol.material.cut_mode = cut if cut else ((), "ANY")
        for tf, cutoff, tint in S.COMPOSITES:
            composite_on(vol, tf, cutoff, tint)
            ref = comp_ref(vol, cam, spec, rings, orac, tf)
            for variant in (0, ROWS, ALWAYS):
                set_variant(vol, variant)
                res = vol.render(cam, spec.width, spec.height, count_steps=True, pick=True)
                torch.cuda.synchronize()
                check_render(res, ref, ("composite", view, linear, bool(cut), tf.size, variant))
            n_hit += int((ref["flags"] == HIT).sum())
    set_variant(vol, 0)
    assert n_hit > 4000
    vol.close()


@pytest.mark.parametrize("linear", [False, True], ids=["nearest", "linear"])
@pytest.mark.parametrize("view", MARCH_VIEWS)
def test_iso_matches_the_twin_and_skipping_changes_nothing(view, linear):
    spec = S.march_spec(view, "mip", "wide-g1-srgb")
    spec.blocked_twin = "all"
    scene = testing.build(spec)
    vol, cam = scene.volume, scene.camera
    W, H = spec.width, spec.height
    orac = lmip.oracle_volume(spec)
    rings = lmip.rings_of(orac)
    vol.material.interpolation = "linear" if linear else "nearest"
    n_hit = skipped = non_finite_normals = 0
    for cut in (None, S.CUT):
        vol.material.cut_planes, vol.material.cut_mode = cut if cut else ((), "ANY")
        for run in S.ISO_RUNS:
            run = dict(run)
            iso_on(vol, run.pop("level"), **run)
            ref = iso_ref(vol, cam, spec, rings, orac)
            frames = []
            for no_skip in (False, True):
                vol.iso_no_skip = no_skip
                out = vol.iso_outputs(W, H, count_steps=True, pick=True, skip_counters=True)
                for name in ("rgba", "depth", "normal"):
                    getattr(out, name).fill_(7.0)
                assert vol.render(cam, W, H, count_steps=True, pick=True, out=out) is out
                torch.cuda.synchronize()
                frames.append((host_iso(out), out.skip_counters.cpu().numpy().view(np.uint32).copy()))
            vol.iso_no_skip = False
            (on, n_on), (off, n_off) = frames
            what = ("iso", view, linear, bool(cut), vol.material.iso_value, run)
            assert_same_planes(on, off, what)
            if cut:                                     # a cut trims stretches with skipping off too (tests/test_gpu_cut.py)
                assert n_on[0] + n_on[1] == n_off[0] + n_off[1] and n_on[1] >= n_off[1], (what, n_on, n_off)
            else:
                assert n_off[1] == 0 and n_on[0] + n_on[1] == n_off[0], (what, n_on, n_off)
                skipped += int(n_on[1])
                if vol.material.iso_value > 0 and view != "inside":    # the one level the host lets skip (iso_value > 0)
                    assert n_on[1] > 0, (what, n_on)
            check_iso(on, ref, what)
            n_hit += int((ref["flags"] == HIT).sum())
            non_finite_normals += int((~np.isfinite(ref["normal"])).any(-1).sum())
    print(view, linear, "iso hits", n_hit, "stretches skipped", skipped, "hits with a non-finite normal", non_finite_normals)
    assert n_hit > 4000
    # Exempt: the inside view.  The single voxels of +-inf and +-3e38 scattered through every LOD leave no 2 x 2 x 2 block
    # of macro cells of the volume below level 25 (70 of LOD 0's 512 cells are, none of their blocks), so a wave skips
    # only where its rays leave the windows: the outside and axis views do (asserted per run above), the inside view's
    # rays start in the middle of LOD 0's window and skipped nothing when measured.
    assert skipped > 0 or view == "inside"
    vol.close()
