"""CPU: the comparison rule every float plane is held to (tests/helpers.py), and the census of the special-value scenes
(tests/special_scenes.py) — from the references alone, each class of fragment that tests/test_gpu_special_values.py
relies on is present at least MIN_FRAGMENTS times in the view and mode built for it.  A count is a condition, not a
measurement: where one is missed the planting moves, not the threshold.  Every count is printed before it is asserted."""
import numpy as np
import pytest

import ortho_scenes as ortho
import special_scenes as S
from composite_twin import composite_twin, material_of
from helpers import assert_close, assert_same_bits, class_error, same_bits_or_nan
from iso_twin import iso_twin
from oracle import lmip, lmip_numpy
from slice_twin import HIT, MISS, twin_of_spec as slice_twin_of

MIN_FRAGMENTS = 30
INF, NAN = np.float32(np.inf), np.float32(np.nan)


# ---- the class rule ---------------------------------------------------------------------------------------------------
def test_class_rule_verdicts():
    """The 3 x 3 table of {finite, +inf, NaN} pairs plus (+inf, -inf): NaN meets NaN, +inf meets +inf, two finite
    values give |a - b|, every other pair is an infinite error."""
    one, two = np.float32(1.0), np.float32(1.25)
    table = [
        (one, two, 0.25), (one, INF, np.inf), (one, NAN, np.inf),
        (INF, one, np.inf), (INF, INF, 0.0), (INF, NAN, np.inf),
        (NAN, one, np.inf), (NAN, INF, np.inf), (NAN, NAN, 0.0),
        (INF, -INF, np.inf), (-INF, -INF, 0.0), (-INF, INF, np.inf),
    ]
    for a, b, want in table:
        assert float(class_error(a, b)) == want, (a, b, want)
    a = np.array([t[0] for t in table], np.float32)
    b = np.array([t[1] for t in table], np.float32)
    assert class_error(a, b).tolist() == [t[2] for t in table]
    # finite values are compared exactly as before: |a - b| in the arguments' own type, the overflow of a difference included
    x, y = np.float32(0.1), np.float32(0.3)
    assert class_error(x, y) == np.abs(x - y)
    assert class_error(np.float32(3e38), np.float32(-3e38)) == np.inf
    # NaN payloads are not pinned: the default NaN of x86 (sign set) meets the one without
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)
    assert (class_error(nans, nans[::-1]) == 0).all() and same_bits_or_nan(nans, nans[::-1]).all()
    # planes compared as bits keep telling -0 from +0 and one finite value from its neighbour
    z = np.array([0.0, -0.0, 1.0], np.float32)
    assert same_bits_or_nan(z, np.array([-0.0, -0.0, np.nextafter(np.float32(1.0), np.float32(2.0))], np.float32)).tolist() == [False, True, False]
    assert same_bits_or_nan(np.array([1, 2], np.uint32), np.array([1, 3], np.uint32)).tolist() == [True, False]
    assert_close(np.array([INF, NAN, 1.0], np.float32), np.array([INF, NAN, 1.0 + 5e-5], np.float32), 1e-4)
    with pytest.raises(AssertionError):
        assert_close(np.array([INF], np.float32), np.array([3e38], np.float32), 1e-4)
    with pytest.raises(AssertionError):
        assert_close(np.array([1.0], np.float32), np.array([1.0 + 2e-4], np.float32), 1e-4)
    with pytest.raises(AssertionError):
        assert_same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))


# ---- the scene --------------------------------------------------------------------------------------------------------
def test_scene_is_what_the_census_assumes():
    d0 = S.pairs()[0][0]
    finite = d0[np.isfinite(d0) & (np.abs(d0) < 1e30)]
    neg = float((finite < 0).mean())
    print("negative share", neg, "min", finite.min(), "max", finite.max())
    assert 0.38 <= neg <= 0.5 and -finite.min() > finite.max()
    for l, (d, lab) in enumerate(S.pairs()):
        assert d.dtype == np.float32 and lab.dtype == np.uint32 and (lab == 0).any()
        bits = d.view(np.uint32)
        for value in S.SINGLES:
            n = int(np.isnan(d).sum()) if np.isnan(value) else int((bits == value.view(np.uint32)).sum())
            assert n >= S.N_SINGLES // 2, (l, value, n)
        b = S.BLOCKS[l]
        assert np.isnan(S._box(d, b["nan_aligned"])).all() and np.isnan(S._box(d, b["nan_straddle"])).all()
        assert all(v % 8 == 0 for v in b["nan_aligned"]) and any(v % 8 for v in b["nan_straddle"])
        block = S._box(d, b["neg_inf"])
        assert ((block == -np.inf) | np.isnan(block)).all() and (block == -np.inf).sum() >= 6 * 64
    spec = S.march_spec("outside", "mip")
    orac = lmip.oracle_volume(spec)
    rois = S.rois(orac)
    assert rois[0][1] == (32, 32, 32) and rois[1][1] == (24, 24, 24) and rois[2][1] == (16, 16, 16)
    for (off, shp), ring in zip(rois[:2], ((32,) * 3, (24,) * 3)):
        assert all(o % r for o, r in zip(off, ring)), (off, ring)          # the window wraps around its ring on every axis
    raw, _ = __import__("sub_volume_renderer_amd").testing.macro_cells_of(np.asarray(S.pairs()[0][0]), 3)
    z0, _, y0, _, x0, _ = S.BLOCKS[0]["nan_aligned"]
    assert raw[z0 // 8, y0 // 8, x0 // 8] == 0.0                            # an all-NaN cell: its maximum is 0


_numpy = {}


def numpy_frame(view, mode):
    if (view, mode) not in _numpy:
        _numpy[(view, mode)] = lmip_numpy.render_spec(S.march_spec(view, mode))
    return _numpy[(view, mode)]


def count(what, n):
    print(what, int(n))
    assert int(n) >= MIN_FRAGMENTS, (what, int(n))


# ---- the march --------------------------------------------------------------------------------------------------------
LMIP_LE0 = ("lmip-30", "lmip0")
INSIDE_RUN = "every inside ray starts in the NaN box at the eye and its run ends within eleven samples, on the +inf box or before it"
INSIDE_WAVG = "every inside ray starts in the NaN box at the eye, so num is NaN: all 7,680 values are NaN (labels and depths stay finite)"
FEW_INF_AT_ENTRY = "a run under a threshold <= 0 starts at the first non-NaN sample and lasts 4 or 11 samples: it ends before a +inf voxel"
# (class, view, mode) -> why the scene cannot hold 30 such fragments; everything else applicable is asserted
EXEMPT = {
    **{("winner +inf", "outside", m): FEW_INF_AT_ENTRY for m in LMIP_LE0}, ("winner +inf", "+x", "lmip0"): FEW_INF_AT_ENTRY,
    **{("winner -inf", "inside", m): INSIDE_RUN for m in ("lmip+20", "lmip-30", "lmip0")},
    **{("winner -0.0 under a threshold <= 0", "inside", m): INSIDE_RUN for m in LMIP_LE0},
    ("winner -0.0 under a threshold <= 0", "+z", "lmip-30"): "rays down +z meet the zero slab 32 voxels after their entry, where their run has ended",
    ("a NaN block passed before the first hit", "inside", "lmip+20"): "the NaN box at the eye is two voxels deep (five samples), then the run begins",
    **{(c, "inside", "wavg"): INSIDE_WAVG for c in ("winner +inf", "winner -inf", "winner negative and finite", "rgba infinite")},
}
BLOCK_SAMPLES = 15      # NaN samples in a row no single voxel or the 4-voxel face patch can give: six voxels of a NaN block or column


def applicable(cls, mode):
    if cls == "winner negative and finite":
        return mode != "lmip+inf"                         # a finite sample never reaches +inf
    if cls == "winner -0.0 under a threshold <= 0":
        return mode in LMIP_LE0
    if cls == "a NaN block passed before the first hit":
        return mode in ("lmip+20", "lmip+inf")            # under a threshold <= 0 a run starts at the first non-NaN sample
    return True


@pytest.mark.parametrize("view", S.VIEWS)
def test_census_of_the_march(view):
    """Every view x mode of the GPU tier x every class that applies to the mode; the exemptions are listed above with
    their reasons, and an exempt count is printed too."""
    for mode in S.MARCH:
        b = numpy_frame(view, mode)
        c = b["census"]
        hit, s = b["flags"] == 2, c["sample"]
        finite_neg = hit & (s < 0) & np.isfinite(s)
        classes = {
            "first executed sample NaN, ray hits": c["first_nan"] & hit,
            "winner +inf": hit & (s == np.inf),
            "winner -inf": hit & (s == -np.inf),
            "winner negative and finite": finite_neg,
            "winner -0.0 under a threshold <= 0": hit & (s == 0) & np.signbit(s),
            "a NaN block passed before the first hit": hit & (c["nan_before"] >= BLOCK_SAMPLES),
            "rgba NaN": np.isnan(b["rgba"]).any(-1),
            "rgba infinite": np.isinf(b["rgba"]).any(-1),
        }
        for cls, mask in classes.items():
            if not applicable(cls, mode):
                continue
            if (cls, view, mode) in EXEMPT:
                print("exempt", (view, mode, cls), int(mask.sum()), EXEMPT[(cls, view, mode)])
                continue
            count((view, mode, cls), mask.sum())
        if mode != "lmip+inf" and (view, mode) != ("inside", "wavg"):
            count((view, mode, "rgba of a negative s"), (finite_neg & np.isfinite(b["rgba"]).all(-1)).sum())
    assert all(v in S.VIEWS and m in S.MARCH for _, v, m in EXEMPT)


@pytest.mark.parametrize("view", S.ORTHO_VIEWS)
def test_census_of_the_axis_views_from_the_columns(view):
    spec = S.march_spec(view, "mip")
    orac = lmip.oracle_volume(spec)
    for mode, thr in (("mip", None), ("first", 20.0), ("first", -30.0)):
        ka = S.column_answers(spec, orac, mode, thr)
        J, v = ka["judged"], ka["value"]
        hit = J & (ka["flags"] == 2)
        what = (view, mode, thr)
        if mode == "mip":
            count((*what, "every voxel of the column NaN: MISS"), (J & (ka["flags"] == 1)).sum())
            count((*what, "winner +inf"), (hit & (v == np.inf)).sum())
            count((*what, "winner -inf"), (hit & (v == -np.inf)).sum())
            count((*what, "winner negative and finite"), (hit & (v < 0) & np.isfinite(v)).sum())
        if thr == 20.0:
            iu, iv = ka["columns"]
            n = 0
            for j, i in zip(*np.nonzero(hit)):
                col = ortho.column_of(ka["val_xyz"], ka["axis"], 1.0, iu[j, i], iv[j, i])
                n += bool(np.isnan(col[:ka["index"][j, i]]).any())
            count((*what, "NaN voxels before the first voxel at the threshold"), n)
    # the all-NaN columns are the planted bundle: exactly its 8 x 8 pixels
    ka = S.column_answers(spec, orac, "mip")
    assert int((ka["judged"] & (ka["flags"] == 1)).sum()) == 64


# ---- slices, slabs, composite, iso --------------------------------------------------------------------------------------
def test_census_of_slices_and_slabs():
    spec = S.march_spec("outside", "mip")
    orac = lmip.oracle_volume(spec)
    W, H = spec.width, spec.height
    total = dict(first=0, later=0, both=0, tie=0, big=0)
    for name, o, u, v in S.planes():
        sl = slice_twin_of(spec, o, u, v, W, H, vol=orac)
        lin = slice_twin_of(spec, o, u, v, W, H, vol=orac, linear=True)
        hit = sl["flags"] == HIT
        count(("slice", name, "non-finite value passed through"), (hit & ~np.isfinite(sl["value"])).sum())
        count(("slice", name, "linear sample with a non-finite corner beside a finite nearest voxel"),
              (hit & np.isfinite(sl["value"]) & ~np.isfinite(lin["value"])).sum())
        vals, held = S.slab_columns(spec, orac, o, u, v, S.SLAB_W[name], 16)
        any_held = held.any(0)
        first = np.argmax(held, axis=0)
        first_val = np.take_along_axis(vals, first[None], 0)[0]
        nan = np.isnan(vals) & held
        total["first"] += int((any_held & np.isnan(first_val)).sum())
        total["later"] += int((any_held & ~np.isnan(first_val) & nan.any(0)).sum())
        total["both"] += int((((vals == np.inf) & held).any(0) & ((vals == -np.inf) & held).any(0)).sum())
        zero = (vals == 0) & held
        best = np.fmax.reduce(np.where(held, vals, -np.inf), axis=0)
        total["tie"] += int(((zero & np.signbit(vals)).any(0) & (zero & ~np.signbit(vals)).any(0) & (best == 0)).sum())
        with np.errstate(over="ignore"):
            total["big"] += int((np.isinf(np.where(held & np.isfinite(vals), vals, 0).astype(np.float32).cumsum(0, dtype=np.float32)).any(0)).sum())
    count(("slab columns of 16", "NaN is the first hit"), total["first"])
    count(("slab columns of 16", "a NaN comes later"), total["later"])
    count(("slab columns of 16", "+inf and -inf meet in a mean"), total["both"])
    count(("slab columns of 16", "-0.0 ties +0.0 at the maximum"), total["tie"])
    print("slab columns of 16 whose running sum overflows", total["big"])


def test_census_of_linear_samples_at_weight_zero():
    """On the centre planes a linear sample inside LOD 0 has every fraction exactly 0: where all eight corners are
    finite it is the nearest voxel, and where a corner of weight 0 is NaN or infinite it is NaN (include/svr.h)."""
    spec = S.march_spec("outside", "mip")
    orac = lmip.oracle_volume(spec)
    total = own = 0
    for name, o, u, v, _ in S.centre_planes():
        near = slice_twin_of(spec, o, u, v, spec.width, spec.height, vol=orac)
        lin = slice_twin_of(spec, o, u, v, spec.width, spec.height, vol=orac, linear=True)
        lod0 = (near["flags"] == HIT) & (near["lod"] == 0)
        both = lod0 & np.isfinite(near["value"]) & np.isfinite(lin["value"])
        assert both.sum() > 500 and (near["value"][both] == lin["value"][both]).all(), name      # every fraction is 0
        zero_weight = lod0 & np.isfinite(near["value"]) & ~np.isfinite(lin["value"])
        assert np.isnan(lin["value"][zero_weight]).all()
        print("centre plane", name, "finite voxels whose linear sample a weight-0 corner made NaN", int(zero_weight.sum()))
        total += int(zero_weight.sum())
        own += int((lod0 & np.isinf(near["value"]) & np.isnan(lin["value"])).sum())
    count(("centre planes", "a corner of weight 0 is NaN or infinite beside a finite voxel"), total)
    count(("centre planes", "an infinite voxel at its own centre gives NaN"), own)


@pytest.mark.parametrize("view", ["outside", "inside", "+y"])
def test_census_of_composite_and_iso(view):
    spec = S.march_spec(view, "mip")
    orac = lmip.oracle_volume(spec)
    rings, M = lmip.rings_of(orac), spec.matrices()
    size, mat = orac.volume_dimensions_shader, material_of(spec.material)
    W, H = spec.width, spec.height
    tf, cutoff, tint = S.COMPOSITES[0]
    ref = composite_twin(rings, M, size, mat, tf.device_table([float(s) for s in size]), W, H, cutoff, tint)
    for k, name in (("nan", "NaN"), ("pinf", "+inf"), ("below", "below 0")):
        count(("composite", view, "a contributing sample is " + name), ref["saw_" + k].sum())
    crossed = bad_gradient = 0
    for run in S.ISO_RUNS:
        p = dict(iso_value=run["level"], refine=run["iso_refine"], color_by_label=run.get("color_by_label", False))
        ref = iso_twin(rings, M, size, mat, W, H, p)
        hit = ref["flags"] == HIT
        crossed += int((hit & (ref["nan_before"] >= 15)).sum())
        bad_gradient += int((hit & ~ref["gradient_finite"]).sum())
        print("iso", view, run["level"], "hits", int(hit.sum()), "misses", int((ref["flags"] == MISS).sum()))
    count(("iso", view, "the level is reached after 15 or more NaN samples (a NaN block was crossed)"), crossed)
    count(("iso", view, "the hit's gradient is not finite"), bad_gradient)
