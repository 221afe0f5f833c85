"""tests/odd_ring_scenes.py held to what tests/test_gpu_odd_rings.py relies on, without a GPU: which row starts every
window visits (expected sets as literals), that the windows wrap, that the x run crosses the x seam inside them, the
share of voxels at LEVEL, the non-finite values of the float rings; and the five twins against references of their own
on these shapes (scipy for components and distance, a triple loop for the objects, a Python loop for the histogram, the
closedness of the mesh), since the GPU module believes the twins."""
import numpy as np
import pytest
from scipy import ndimage

import odd_ring_scenes as S
from components_twin import components_twin
from distance_twin import FAR, distance_twin
from histogram_twin import histogram_twin
from mesh_twin import mesh_twin
from objects_twin import brute_force, objects_twin
from test_components import STRUCTURE, by_label_with_scipy
from test_distance import scipy_squared
from test_mesh import closed_and_oriented

f32 = np.float32
ALL4, ALL8, ALL16 = set(range(4)), set(range(8)), set(range(16))
# Row starts modulo 4 (the unit of the components, distance, mesh and objects passes), by the window's first x slot
# modulo 4: the rows of the pieces that begin at that slot and of the pieces that wrapped to slot 0
UNIT_HEADS = {
    "odd3": [ALL4, ALL4, ALL4, ALL4], "odd1": [ALL4, ALL4, ALL4, ALL4], "thin3": [ALL4, ALL4, ALL4, ALL4], "thin1": [ALL4, ALL4, ALL4, ALL4],
    "even2": [{0, 2}, ALL4, {0, 2}, ALL4],
    "quad": [{0}, {0, 1}, {0, 2}, {0, 3}], "oct": [{0}, {0, 1}, {0, 2}, {0, 3}],
}
# Row starts modulo the elements of a 16-byte slot of the density ring (the histogram), by (geometry, elements per slot)
# and the window's first x slot modulo 8
SLOT_HEADS = {
    ("odd3", 16): [ALL16] * 8, ("odd3", 8): [ALL8] * 8, ("odd3", 4): [ALL4] * 8, ("odd1", 4): [ALL4] * 8, ("odd1", 16): [ALL16] * 8,
    ("thin3", 16): [ALL16] * 8, ("thin1", 16): [ALL16] * 8,
    ("even2", 8): [{0, 2, 4, 6}, ALL8] * 4,
    ("quad", 16): [{0, 4, 8, 12}, {0, 1, 4, 5, 8, 9, 12, 13}, {0, 2, 4, 6, 8, 10, 12, 14}, {0, 3, 4, 7, 8, 11, 12, 15}] * 2,
    ("oct", 16): [{0, 8}, {0, 1, 8, 9}, {0, 2, 8, 10}, {0, 3, 8, 11}, {0, 4, 8, 12}, {0, 5, 8, 13}, {0, 6, 8, 14}, {0, 7, 8, 15}],
}
# windows of fewer rows than there are row starts: a subset of the literal set, and more than one start
FEW_ROWS = {("quad", "part"), ("thin3", "part"), ("thin1", "part")}
FAR_WRAPS = {"odd3": (True, True, False), "even2": (True, True, False)}       # 2^31 - 1 - shape lands on ring slot 0 on z


def every_window(keys=None):
    for key in keys or S.SCENES:
        sc = S.scene(key)
        for li, lod in enumerate(sc.lods):
            for name, off, shape in S.windows(lod.geometry):
                yield sc, li, lod, name, off, shape


def test_the_scenes_are_the_ones_asked_for():
    assert S.RINGS == {"odd3": (63, 15, 25), "odd1": (21, 7, 9), "even2": (42, 12, 10), "quad": (36, 6, 5), "oct": (40, 5, 6),
                       "thin3": (3, 5, 7), "thin1": (1, 4, 6)}
    assert [r[0] % 16 for r in S.RINGS.values()] == [15, 5, 10, 4, 8, 3, 1]
    assert all(np.prod(r) <= 25000 for r in S.RINGS.values())
    assert {k: v[1:] for k, v in S.SCENES.items() if v[0] == ["odd3"]} == {
        "odd3-u8": ("uint8", True), "odd3-u16": ("uint16", True), "odd3-f32": ("float32", True), "odd3-nolabels": ("uint8", False)}
    assert sorted(v[0][0] for v in S.SCENES.values() if len(v[0]) == 1) == sorted(["odd3"] * 4 + ["odd1", "even2", "quad", "oct", "thin3", "thin1"])
    assert S.SCENES["odd3+odd1-u8"][0] == ["odd3", "odd1"] and 63 * 15 * 25 % 2 == 1      # LOD 1 follows an odd number of voxels
    for sc, li, lod, name, off, shape in every_window():
        assert lod.density.dtype == S.DTYPE[sc.storage] and lod.density.shape == lod.ring[::-1]
        assert (lod.labels is None) == (not sc.has_labels)
        assert all(0 <= o and o + n <= 2 ** 31 - 1 and 1 <= n <= r for o, n, r in zip(off, shape, lod.ring))
    names = {g: [n for n, _, _ in S.windows(g)] for g in S.RINGS}
    assert all(names[g] == ["full0", "full1", "full2", "full3", "part"] + (["far"] if g in ("odd3", "even2") else []) for g in S.RINGS)


def test_windows_are_where_the_issue_puts_them():
    for geometry, ring in S.RINGS.items():
        wins = {name: (off, shape) for name, off, shape in S.windows(geometry)}
        for k in range(4):
            off, shape = wins[f"full{k}"]
            assert shape == ring and off[0] % 4 == k
            assert all(off[a] % ring[a] != 0 for a in range(3) if ring[a] > 1), (geometry, k)
        off, shape = wins["part"]
        assert shape == tuple(max(r - c, 1) for r, c in zip(ring, (5, 2, 3)))
        assert S.wraps(ring, off, shape) == tuple(n > 1 for n in shape), geometry       # on all three axes where its shape allows
        if "far" in wins:
            off, shape = wins["far"]
            assert shape == wins["part"][1] and off == tuple(2 ** 31 - 1 - n for n in shape)
            assert S.wraps(ring, off, shape) == FAR_WRAPS[geometry]
    for sc, li, lod, name, off, shape in every_window():
        if name.startswith("full"):
            assert S.wraps(lod.ring, off, shape) == tuple(r > 1 for r in lod.ring)


def test_every_window_visits_the_row_starts_its_pitch_can_produce():
    units = {}
    for sc, li, lod, name, off, shape in every_window():
        s0 = off[0] % lod.ring[0]
        per = S.PER_SLOT[sc.storage]
        for modulus, want in ((4, UNIT_HEADS[lod.geometry][s0 % 4]), (per, SLOT_HEADS[(lod.geometry, per)][s0 % 8])):
            by_piece = S.row_starts(lod.ring, off, shape, modulus)
            got = set().union(*by_piece)
            what = (sc.key, li, name, modulus, sorted(got), sorted(want))
            if (lod.geometry, name) in FEW_ROWS:
                assert got <= want and len(got) >= 2, what
            else:
                assert got == want, what
            if lod.ring[0] % 4 and name.startswith("full"):          # the start varies from row to row inside one piece
                assert max(len(p) for p in by_piece) >= (2 if lod.ring[0] % 2 == 0 or lod.ring[0] == 1 else 4), what
        units.setdefault((sc.key, li), set()).update(*S.row_starts(lod.ring, off, shape, 4))
    assert all(u == ALL4 for u in units.values()), units              # the four W-full offsets reach every start on any pitch
    # the unaligned whole unit: on the odd pitches a row of the window begins 1, 2 or 3 elements into a unit while the
    # row is long enough to hold whole units behind it
    for geometry in ("odd3", "odd1", "even2"):
        name, off, shape = S.windows(geometry)[4]
        assert shape[0] >= 16 and len(set().union(*S.row_starts(S.RINGS[geometry], off, shape, 4))) == 4


def test_windows_sit_where_a_plan_one_slot_short_would_miss_voxels():
    """The lanes that share a row visit a power of two of slots (or a multiple of 8): a plan that counted a row's slots
    too low by one is hidden wherever the count is no such boundary.  The W-full windows are put where it is, for the
    unit of 4 and for every slot size the pitch allows; where the row start cannot vary (4 | x for the unit) nothing can."""
    assert [S.slots_covered(k) for k in (1, 2, 3, 4, 5, 8, 9, 16, 17)] == [1, 2, 4, 4, 8, 8, 16, 16, 24]
    want = {"odd3": {4, 8, 16}, "odd1": {4, 8, 16}, "even2": {4, 8, 16}, "quad": {8, 16}, "oct": {16}, "thin3": {4, 8, 16}, "thin1": set()}
    for geometry, ring in S.RINGS.items():
        got = set()
        per_window = []
        for name, off, shape in S.windows(geometry)[:4]:
            mine = {per for per in (4, 8, 16) for (s, _, _), (n, _, _) in S.pieces_of(ring, off, shape) if S.last_slot_matters(ring[0], s, n, per)}
            per_window.append(mine)
            got |= mine
        assert got == want[geometry], (geometry, got)
        if geometry in ("odd3", "odd1", "even2", "thin3"):
            assert all(w == {4, 8, 16} for w in per_window), (geometry, per_window)
    # the rule itself, on a row of 30 voxels at slot 0 of the 63-voxel ring: 8 slots of 4 if it began a slot, 9 three voxels in
    assert S.last_slot_matters(63, 0, 30, 4) and not S.last_slot_matters(63, 0, 20, 4) and not S.last_slot_matters(36, 0, 30, 4)


def test_the_x_run_crosses_the_seam_inside_every_window():
    seen = 0
    for sc, li, lod, name, off, shape in every_window():
        length = S.run_of(lod.ring[0])[0]
        if not sc.has_labels or not length or name == "far":
            continue
        off, shape, ring, dens, labs = lod.window(off, shape)
        run, first = S.longest_x_run(labs, S.RUN_LABEL)
        assert run == length >= 12, (sc.key, name, run)
        seam = lod.ring[0] - off[0] % lod.ring[0]                      # the window's x at which the ring wraps
        assert first + 4 <= seam <= first + run - 4, (sc.key, name, first, seam)
        seen += 1
    assert S.run_of(63)[0] == 40 and seen >= 40
    # W-far is where the issue puts it: what it holds of the run still crosses the seam on odd3
    off, shape, ring, dens, labs = S.scene("odd3-u8").lods[0].window(*S.windows("odd3")[5][1:])
    run, first = S.longest_x_run(labs, S.RUN_LABEL)
    assert run >= 16 and first < 63 - off[0] % 63 < first + run


def test_content():
    for key in S.SCENES:
        sc = S.scene(key)
        for lod in sc.lods:
            with np.errstate(invalid="ignore"):
                share = float((lod.density >= S.DTYPE[sc.storage](S.LEVEL[sc.storage])).mean())
            assert 0.3 < share < 0.7, (key, share)
            if lod.labels is not None:
                ids = set(np.unique(lod.labels).tolist())
                assert {0, 9, 10, 1} <= ids <= {0, 9, 10, 1, 2, 3, 0xFFFFFFF0}
                assert ids == {0, 9, 10, 1, 2, 3, 0xFFFFFFF0} or lod.ring[0] < 20
    for sc, li, lod, name, off, shape in every_window():
        off, shape, ring, dens, labs = lod.window(off, shape)
        assert dens.dtype == f32 and dens.shape == tuple(shape[::-1])
        if dens.size >= 64:                                            # a window of a few voxels is whatever its voxels are
            with np.errstate(invalid="ignore"):
                share = float((dens >= f32(S.LEVEL[sc.storage])).mean())
            assert 0.3 < share < 0.7, (sc.key, name, share)
        if sc.storage == "float32":
            assert np.isnan(dens).any() and np.isposinf(dens).any() and np.isneginf(dens).any(), (sc.key, name)
        if labs is not None and lod.ring[0] >= 20:                     # (the boxes fill most of a thin ring)
            assert (labs == 1).any() and (np.isin(labs, [9, 10])).mean() > 0.4
    lo, hi = S.scene("odd3-f32").lods[0].tails_range()
    assert np.isfinite([lo, hi]).all()


def test_boxes_are_the_ones_asked_for():
    name, off, shape = S.windows("odd3")[4]
    ring = S.RINGS["odd3"]
    boxes = dict(S.boxes(off, shape, ring))
    seam = ring[0] - off[0] % ring[0]
    assert boxes["window"] is None and len(boxes) == 1 + 5 * 6 + 4
    for nx in (1, 3, 4, 5, 33):
        for start in (0, 1, 2, 3, seam - 2, seam - 1):
            o, n = boxes[f"row {nx} at {start}"]
            assert o[0] == off[0] + start and n[0] == nx and o[0] + nx <= off[0] + shape[0]
            assert S.wraps(ring, o, n)[1:] == (True, True)
    assert {(off[0] + s) % 63 % 4 for s in (0, 1, 2, 3)} == ALL4 and (off[0] + seam) % 63 == 0
    assert [boxes[k][1].index(1) for k in ("thin x", "thin y", "thin z")] == [0, 1, 2]
    o, n = boxes["partly outside"]
    assert o[0] < off[0] and o[1] + n[1] > off[1] + shape[1] and o[2] + n[2] > off[2] + shape[2]
    assert len(S.plan_cases()) == sum(len(S.windows(g)) for g in S.RINGS) + len(boxes) - 1


# ---- the twins on these shapes ---------------------------------------------------------------------------------------------
PART_AND_FAR = [(sc.key, li, name) for sc, li, lod, name, off, shape in every_window() if not name.startswith("full")]


def window_of(key, li, name):
    sc = S.scene(key)
    lod = sc.lods[li]
    off, shape = {n: (o, s) for n, o, s in S.windows(lod.geometry)}[name]
    return sc, lod, off, shape


@pytest.mark.parametrize("key,li,name", PART_AND_FAR)
def test_components_and_distance_twins_are_scipys(key, li, name):
    sc, lod, off, shape = window_of(key, li, name)
    off, shape, ring, dens, labs = lod.window(off, shape)
    level = S.LEVEL[sc.storage]
    with np.errstate(invalid="ignore"):
        inside = dens >= f32(level)
    for connectivity in (6, 26):
        twin = components_twin(off, dens, labs, level=level, connectivity=connectivity)
        want, count = ndimage.label(inside, structure=STRUCTURE[connectivity])
        assert twin["header"][0] == count and np.array_equal(twin["ids"], want), (key, name, connectivity)
        assert twin["header"][4:13] == [*off, *off, *shape]
        if labs is not None:
            picked = np.isin(labs, S.SELECTED)
            twin = components_twin(off, dens, labs, selected=S.SELECTED, connectivity=connectivity)
            want, count = by_label_with_scipy(labs, picked, connectivity)
            assert twin["header"][:2] == [count, int(picked.sum())] and np.array_equal(twin["ids"], want), (key, name, connectivity)
    for invert in (False, True):
        target = ~inside if invert else inside
        twin = distance_twin(off, dens, labs, level=level, invert=invert)
        if (~target).any():
            assert np.array_equal(twin["d2"], scipy_squared(target)), (key, name, invert)
        else:
            assert (twin["d2"] == FAR).all()
        twin = distance_twin(off, dens, labs, level=level, invert=invert, border=True)
        want = scipy_squared(np.pad(target, 1, constant_values=False))[1:-1, 1:-1, 1:-1] if not invert else None
        if want is not None:
            assert np.array_equal(twin["d2"], want), (key, name, "border")
        assert twin["header"][4:13] == [*off, *off, *shape]


def histogram_by_hand(values, lo, hi, bins):
    lo, hi = f32(lo), f32(hi)
    inv = f32(bins) / (hi - lo)
    counts, tail = [0] * bins, [0, 0, 0, 0]
    for v in values.reshape(-1):
        tail[3] += 1
        if v != v:
            tail[2] += 1
        elif v < lo:
            tail[0] += 1
        elif v > hi:
            tail[1] += 1
        else:
            counts[min(int(f32(v - lo) * inv), bins - 1)] += 1
    return counts, tail


@pytest.mark.parametrize("key,li,name", PART_AND_FAR)
def test_histogram_objects_and_mesh_twins(key, li, name):
    sc, lod, off, shape = window_of(key, li, name)
    ring = lod.ring_dict(off, shape)
    off, shape, _, dens, labs = lod.window(off, shape)
    lo, hi = lod.tails_range()
    for bins in (7, 256):
        twin = histogram_twin({li: ring}, li, lo, hi, bins)
        counts, tail = histogram_by_hand(dens, lo, hi, bins)
        assert twin["counts"].tolist() == counts and twin["tail"].tolist() == tail, (key, name, bins)
        real = dens[~np.isnan(dens)]
        assert twin["range"].tolist() == [real.min(), real.max()]
    picked = S.selections(sc.has_labels)[0]
    if labs is not None:
        twin = histogram_twin({li: ring}, li, lo, hi, 7, labels=picked)
        counts, tail = histogram_by_hand(dens[np.isin(labs, picked)], lo, hi, 7)
        assert twin["counts"].tolist() == counts and twin["tail"].tolist() == tail
    # the objects: a triple loop on the integer rings; per-label masks on the float ones (the loop reads whole numbers)
    for labels, ignore_zero in ((None, False), (picked, False), (None, True)):
        twin = objects_twin(ring, None, labels, ignore_zero, integer=sc.storage != "float32")
        if sc.storage != "float32":
            want = brute_force(ring, None, labels, ignore_zero)
            assert twin["header"] == want["header"] and sorted(twin["objects"]) == sorted(want["objects"]), (key, name)
            for label, rec in twin["objects"].items():
                ref = want["objects"][label]
                assert all(rec[k] == ref[k] for k in ("voxels", "finite", "value_sum", "vmin", "vmax")), (key, name, label)
                assert all(list(rec[k]) == list(ref[k]) for k in ("sum", "lo", "hi")), (key, name, label)
        else:
            z, y, x = np.meshgrid(*[np.arange(n) for n in dens.shape], indexing="ij")
            for label, rec in twin["objects"].items():
                m = labs == label
                fin = dens[m][np.isfinite(dens[m])]
                assert (rec["voxels"], rec["finite"]) == (int(m.sum()), fin.size) and not (ignore_zero and label == 0)
                assert list(rec["sum"]) == [int(x[m].sum()), int(y[m].sum()), int(z[m].sum())]
                assert list(rec["lo"]) == [off[0] + x[m].min(), off[1] + y[m].min(), off[2] + z[m].min()]
                assert rec["vmin"] == (fin.min() if fin.size else np.inf) and abs(rec["value_sum"] - float(fin.astype(np.float64).sum())) <= 1e-9 * rec["abs_sum"]
            assert twin["header"][1] == int(np.isin(labs, list(twin["objects"])).sum())
    # the mesh: closed, oriented, and around exactly the inside voxels
    for mode in (dict(selected=picked), dict(level=S.LEVEL[sc.storage])):
        twin = mesh_twin(off, dens, labs, **mode)
        with np.errstate(invalid="ignore"):
            inside = dens >= f32(mode["level"]) if "level" in mode else np.isin(np.zeros(dens.shape, np.uint32) if labs is None else labs, picked)
        assert twin["header"][7] == int(inside.sum()) and twin["header"][4:7] == list(off)
        closed_and_oriented(twin["vertices"], twin["triangles"])
        assert len(twin["triangles"]) > 0 or not inside.any()
