"""CPU tier of the mode fuzz (tools/fuzz_modes.py; the device half is tests/test_gpu_mode_fuzz.py), from the twins alone.
Pins: ``random_case(seed)`` is a record like ``fuzz_parity.random_spec`` - sha256 digests of the scene and of every
mode parameter of a handful of seeds.  Census: over exactly the seeds the GPU test replays, every block has enough
cases with hits for each entry point and every feature the draw is meant to exercise occurs.  Sensitivity: the twins'
outputs on inputs perturbed in one place differ from those on the drawn inputs, under the comparison the GPU test makes
(tools/fuzz_modes.compare), in at least 10 % of the seeds where the perturbation applies: a floor against a draw that
never exercises a feature, not a measurement.  Each figure is printed before it is asserted."""
import dataclasses
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_modes as F  # noqa: E402
from test_fuzz_spec_pins import _plain, spec_digest  # noqa: E402

HIT, MISS = 2, 1
MODE_KEYS = ("interpolation", "slice", "slab", "composite", "iso", "cut")


def case_digest(case):
    """``spec_digest`` of the scene, extended by the mode parameters."""
    h = hashlib.sha256(spec_digest(case["spec"], case["region"], case["variant"]).encode())
    h.update(repr(_plain({k: case[k] for k in MODE_KEYS})).encode())
    return h.hexdigest()


PINNED = {
    (0, False): "bbe8a47f34cc67a8fb185ad56c9fd5107548e3310d0c824c7bb20719f0c03f37",
    (1, True): "3f987a94cf619d566fdf21e34086e7c92b9aa175be9920608c9b66a424b201aa",
    (7064, False): "89dfe2ce847a389768f918859d3a2551f563e310b84a62cf1bf0176aa2befc9a",
    (7121, False): "fe4caeff2ae934815160beba5eee20dd7ca58fc3b01c8586a4562b7e0329e7d8",
    (7183, False): "64aefd5e4d6ad4df7d7b43127263e71c06b7b8f8248e33edf8f4582369f22631",
    (7064, True): "e3fab11ec5b94c8731c74d34dda4e3418a1e4e7d8a71b859f85ffbc197abc184",
    (7103, True): "20919635708cef0151f159372c0547f42e8e526244728b2a3d7edb45c506144e",
    (9041, False): "771e1f2765ebf2d093f059afe67b218cce54f23ddd266d42eb1ec1d40fb142bb",
}


@pytest.mark.parametrize("seed,ortho", sorted(PINNED))
def test_a_seed_names_one_case_for_good(seed, ortho):
    case = F.random_case(seed, ortho)
    print(seed, ortho, case_digest(case))
    assert case_digest(case) == PINNED[(seed, ortho)]


def test_the_mode_draw_leaves_the_scene_as_random_spec_draws_it():
    for seed, ortho in ((7067, False), (7075, True)):
        case = F.random_case(seed, ortho)
        spec, region, variant = F.fuzz_parity.random_spec(seed, ortho=ortho)
        assert case["variant"] == variant & 0x300 and case["region"] == region
        # the fields of the spec the mode draw sets: the copy policy, and clim[1] where bounded_clim raises it
        spec.blocked_twin = case["spec"].blocked_twin
        (lo, hi), (mine_lo, mine_hi) = spec.material["clim"], case["spec"].material["clim"]
        assert mine_lo == lo and mine_hi >= hi
        spec.material["clim"] = case["spec"].material["clim"]
        assert spec_digest(spec, region, 0) == spec_digest(case["spec"], region, 0)


# ---- the suite's seeds, each run once ------------------------------------------------------------------------------------
_RECORDS = {}


def record(seed, ortho):
    """The case, its twin inputs and the twins' outputs, computed once per seed and left unchanged."""
    key = (seed, ortho)
    if key not in _RECORDS:
        case = F.random_case(seed, ortho)
        T = F.twin_inputs(case)
        _RECORDS[key] = (case, T, F.run_twins(T))
    return _RECORDS[key]


def block_seeds(first, ortho):
    return [(seed, ortho) for seed in range(first, first + F.SUITE_BLOCK)]


def region_kind(region):
    if region is None:
        return "full"
    return "tile" if region.band_pitch == region.out_h and region.band_h == region.out_h else "stripes"


def test_census_of_the_seeds_the_gpu_test_replays():
    assert len(F.SUITE_BLOCKS) == 16 and sum(not o for _, o in F.SUITE_BLOCKS) == 12
    seen = {k: set() for k in ("slab", "interpolation", "cut", "tint", "refine", "light", "region", "dtype", "labels",
                               "copies", "lods", "selected", "alpha")}
    no_grid = comp_hit_iso_miss = all_miss_composite = 0
    for first, ortho in F.SUITE_BLOCKS:
        enough = dict.fromkeys(F.ENTRY_POINTS, 0)
        for seed, _ in block_seeds(first, ortho):
            case, T, refs = record(seed, ortho)
            for k, n in F.hit_counts(refs).items():
                enough[k] += n >= 100
            spec, cut = case["spec"], case["cut"]
            seen["slab"].add(case["slab"]["mode"])
            seen["interpolation"].add(case["interpolation"])
            seen["cut"].add("none" if not cut["planes"] else "8" if len(cut["planes"]) == 8 else cut["mode"])
            seen["tint"] |= {("composite", case["composite"]["color_by_label"]), ("iso", case["iso"]["color_by_label"])}
            seen["refine"].add(min(case["iso"]["iso_refine"], 2))
            seen["light"].add(case["iso"]["light_direction"] is None)
            seen["region"].add(region_kind(case["region"]))
            seen["dtype"].add(str(spec.pairs[0][0].dtype))
            seen["labels"].add(spec.pairs[0][1] is not None)
            seen["copies"].add(spec.blocked_twin)
            seen["lods"].add(len(spec.pairs))
            seen["alpha"].add(case["composite"]["alpha_shape"])
            if "slice" in refs:
                seen["selected"] |= set(np.unique(refs["slice"]["lod"]).tolist())
            no_grid += any(n % 8 for r in T["rings"] for n in np.asarray(r["density"]).shape)
            comp, iso = refs["composite"]["flags"], refs["iso"]["flags"]
            comp_hit_iso_miss += bool(((comp == HIT) & (iso == MISS)).any())
            all_miss_composite += bool((comp == MISS).any() and not (comp == HIT).any())
        print("block", first, "ortho" if ortho else "perspective", "seeds with >= 100 HIT pixels", enough)
        assert all(3 * n >= F.SUITE_BLOCK for n in enough.values()), (first, ortho, enough)
    print("census", {k: sorted(v, key=str) for k, v in seen.items()}, "cases with a ring that has no macro-cell grid", no_grid,
          "with a composite hit on an iso MISS", comp_hit_iso_miss, "with an all-MISS composite", all_miss_composite)
    assert seen["slab"] == {"max", "min", "mean"} and seen["interpolation"] == {"nearest", "linear"}
    assert seen["cut"] == {"none", "ANY", "ALL", "8"}
    assert seen["tint"] == {(m, t) for m in ("composite", "iso") for t in (False, True)}
    assert seen["refine"] == {0, 1, 2} and seen["light"] == {False, True}
    assert seen["region"] == {"full", "tile", "stripes"}
    assert seen["dtype"] == {"uint8", "uint16", "float32"} and seen["labels"] == {False, True}
    assert seen["copies"] == {"auto", "all", False} and seen["lods"] == {1, 2, 3, 4}
    assert seen["selected"] >= {0, 1, 2, 3}
    assert seen["alpha"] == {"ramp", "step", "spikes", "zero", "opaque"}
    assert no_grid >= 1 and comp_hit_iso_miss >= 1 and all_miss_composite >= 1


# ---- sensitivity -------------------------------------------------------------------------------------------------------------
def _with_ring(T, lod, **changed):
    rings = list(T["rings"])
    rings[lod] = dict(rings[lod], **changed)
    return dict(T, rings=rings)


def _moved_offset(T, seed):
    lod, axis = seed % len(T["rings"]), seed % 3
    offset = list(T["rings"][lod]["offset"])
    offset[axis] += 1
    return _with_ring(T, lod, offset=tuple(offset))


def _rolled_density(T, seed):
    lod = seed % len(T["rings"])
    return _with_ring(T, lod, density=np.roll(np.asarray(T["rings"][lod]["density"]), 1, axis=2))


def _moved_plane(T, seed):
    planes = [list(p) for p in T["cut_planes"]]
    planes[seed % len(planes)][3] += 0.5 * float(np.mean(np.abs(np.diag(np.linalg.inv(T["world_inv"]))[:3])))
    return dict(T, cut_planes=[tuple(p) for p in planes])


def _changed_alpha(T, seed):
    table = np.array(T["table"])
    j = len(table) // 2
    table[j, 3] = (table[j, 3] + np.float32(0.37)) % np.float32(1.0)
    return dict(T, table=table)


def _changed_band(T, seed):
    r = T["region"]
    band = r.band_h or r.out_h
    return dict(T, region=dataclasses.replace(r, band_h=band // 2 if band > 1 else 2, band_pitch=r.band_pitch or r.out_h))


ALL = F.ENTRY_POINTS
RAYS = ("composite", "iso")
# name, the twins it reaches, where it applies, the perturbed inputs
PERTURBATIONS = [
    ("ring offset + 1 on one axis", ALL, lambda T: True, _moved_offset),
    ("density rolled by one texel along x", ALL, lambda T: True, _rolled_density),
    ("linear flipped", ALL, lambda T: True, lambda T, s: dict(T, linear=not T["linear"])),
    ("a cut plane's d moved by half a voxel", RAYS, lambda T: len(T["cut_planes"]) > 0, _moved_plane),
    ("cut_mode flipped", RAYS, lambda T: len(T["cut_planes"]) > 1,
     lambda T, s: dict(T, cut_mode="ALL" if T["cut_mode"] == "ANY" else "ANY")),
    ("one table entry's alpha changed", ("composite",), lambda T: True, _changed_alpha),
    ("refine + 1", ("iso",), lambda T: T["iso"]["refine"] < 16, lambda T, s: dict(T, iso=dict(T["iso"], refine=T["iso"]["refine"] + 1))),
    ("slab samples + 1", ("slab",), lambda T: F.plane_region_fits(T["region"], T["width"], T["height"]),
     lambda T, s: dict(T, slab=dict(T["slab"], samples=T["slab"]["samples"] + 1))),
    ("the region's band_h changed", ALL, lambda T: T["region"] is not None, _changed_band),
]
# the first two perspective blocks and the first orthographic one
SENSITIVITY_SEEDS = [s for first, ortho in F.SUITE_BLOCKS[:2] + F.SUITE_BLOCKS[12:13] for s in block_seeds(first, ortho)]


@pytest.mark.parametrize("name,which,applies,perturb", PERTURBATIONS, ids=[p[0] for p in PERTURBATIONS])
def test_the_comparison_detects_a_perturbation(name, which, applies, perturb):
    applied = detected = 0
    for seed, ortho in SENSITIVITY_SEEDS:
        _, T, refs = record(seed, ortho)
        if not applies(T):
            continue
        applied += 1
        moved = F.run_twins(perturb(T, seed), which)
        base = {k: refs[k] for k in which if k in refs}
        detected += set(moved) != set(base) or any(F.compare(k, moved[k], base[k]) is not None for k in base)
    print(f"{name}: detected in {detected} of the {applied} seeds where it applies ({100.0 * detected / max(applied, 1):.0f} %)")
    assert applied >= 5 and 10 * detected >= applied, (name, detected, applied)
