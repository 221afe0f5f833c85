"""GPU: svr_histogram (include/svr.h) == the numpy restatement of tests/histogram_twin.py, ``array_equal`` on counts and
tail, min and max by value: u8 / u16 / float32 rings (the float source seeded with NaN, +-inf and negative values), 1 ..
4096 bins, ranges with tails and with ``hi`` on a data value, boxes across the wrap seams / with odd x spans / partly and
wholly outside the window / of one voxel, a LOD without a window, label filters (with and without label rings), a
constant ring (the contended path), a moving window, the micro-block copy, the Python surface (box mapping, default
ranges, ``auto_clim``), untouched renders, and every refusal with nothing enqueued."""
import ctypes as C

import numpy as np
import pytest
import torch

from histogram_twin import (auto_clim_twin, considered_texels, edges_twin, histogram_twin, lod_box_twin)
from oracle import lmip
from sub_volume_renderer_amd import _native as N, testing

pytestmark = pytest.mark.gpu
f32 = np.float32
BINS = (1, 2, 7, 256, 4096)
WINDOW0 = 48 * 40 * 40


def spec_of(kind):
    spec = testing.synthetic_spec(64, 96, 80)
    if kind == "u16":
        spec.pairs = [(d.astype(np.uint16) * np.uint16(251), l) for d, l in spec.pairs]
    if kind == "f32":
        pairs = []
        for k, (d, l) in enumerate(spec.pairs):
            d = d.astype(f32) * f32(0.37) - f32(20.0)                     # negative values too
            flat = d.reshape(-1)
            # the special values go into unlabelled voxels only, so that every labelled object stays finite
            free = np.flatnonzero(np.asarray(l).reshape(-1) == 0)
            if free.size < 650:                                           # the coarsest level: it never has a window
                pairs.append((d, l))
                continue
            pick = np.random.default_rng(10 + k).choice(free, 650, replace=False)
            flat[pick[:200]], flat[pick[200:400]], flat[pick[400:600]] = np.nan, np.inf, -np.inf
            flat[pick[600:]] = f32(3e38)                                  # v - lo overflows under a range as wide as f32
            pairs.append((d, l))
        spec.pairs = pairs
    if kind == "nolabels":
        spec.pairs = [(d, None) for d, _ in spec.pairs]
    if kind == "twin_all":
        spec.blocked_twin = "all"
    if kind == "twin_off":
        spec.blocked_twin = False
    return spec


_SCENES = {}


def scene_of(kind):
    """(volume, rings of the CPU restatement) of a scene, built once per module run."""
    if kind not in _SCENES:
        spec = spec_of(kind)
        vol = testing.build(spec).volume
        assert vol._rings.density_storage == {"u16": "uint16", "f32": "float32"}.get(kind, "uint8")
        _SCENES[kind] = (vol, lmip.rings_of(lmip.oracle_volume(spec)))
    return _SCENES[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    """The shared scenes free their rings when the module's tests are done."""
    yield
    for vol, _ in _SCENES.values():
        vol.close()
    _SCENES.clear()


def c_hist(vol, lod, lo, hi, bins, box=None, labels=None):
    """One svr_histogram call through the C ABI into sentinel-filled buffers -> dict of numpy arrays."""
    handle = vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    counts = torch.full((bins,), -7, dtype=torch.int64, device=dev)
    tail = torch.full((4,), -7, dtype=torch.int64, device=dev)
    rng = torch.full((2,), 7.0, dtype=torch.float32, device=dev)
    hp = N.HistogramParams(lod=lod, lo=lo, hi=hi, bins=bins)
    if box is not None:
        hp.use_box = 1
        hp.box_off[:], hp.box_shape[:] = box
    sel = None
    if labels is not None:
        sel = torch.from_numpy(np.unique(np.asarray(labels, np.uint32)).view(np.int32)).to(dev)
        hp.selected, hp.selected_count = sel.data_ptr(), sel.numel()
    ho = N.HistogramOutputs(counts.data_ptr(), tail.data_ptr(), rng.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.lib().svr_histogram(handle, C.byref(hp), C.byref(ho), C.c_void_p(stream)), "svr_histogram")
    torch.cuda.synchronize()
    return dict(counts=counts.cpu().numpy().view(np.uint64), tail=tail.cpu().numpy().view(np.uint64), range=rng.cpu().numpy())


def same(got, ref, what):
    assert np.array_equal(got["counts"], ref["counts"]), (what, "counts", np.flatnonzero(got["counts"] != ref["counts"])[:8])
    assert np.array_equal(got["tail"], ref["tail"]), (what, "tail", got["tail"], ref["tail"])
    assert got["range"][0] == ref["range"][0] and got["range"][1] == ref["range"][1], (what, got["range"], ref["range"])


def ranges_of(values):
    """The type's whole range, and one with non-empty tails whose hi is a data value."""
    real = np.unique(values[np.isfinite(values)])
    lo, hi = float(real[real.size // 4]) + 0.25, float(real[3 * real.size // 4])
    assert real.size > 16 and (real < lo).any() and (real > hi).any() and (real == f32(hi)).any()
    return lo, hi


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_storage_bins_and_ranges(kind):
    vol, rings = scene_of(kind)
    full = {"u8": (0.0, 256.0), "u16": (0.0, 65536.0), "f32": (-120.0, 75.0)}[kind]
    for lod in (0, 1):
        values = considered_texels(rings[lod])
        assert values.size == (WINDOW0 if lod == 0 else 32 ** 3)
        tails = ranges_of(values)
        for bins in BINS:
            for lo, hi in (full, tails):
                ref = histogram_twin(rings, lod, lo, hi, bins)
                same(c_hist(vol, lod, lo, hi, bins), ref, (kind, lod, bins, lo, hi))
                if (lo, hi) == tails:
                    assert ref["tail"][0] > 0 and ref["tail"][1] > 0 and ref["counts"][bins - 1] > 0
        if kind == "f32":
            assert ref["tail"][2] > 0 and ref["range"][0] == -np.inf and ref["range"][1] == np.inf
            # a range whose width overflows f32: inv == 0, and for v = 3e38 the product inf * 0 is NaN -> bin 0 (svr.h)
            for bins in (1, 4):
                ref = histogram_twin(rings, lod, -3e38, 3e38, bins)
                same(c_hist(vol, lod, -3e38, 3e38, bins), ref, (kind, lod, bins, "f32-wide"))
                assert ref["counts"][0] == ref["counts"].sum() > 0 and ref["tail"][0] > 0 and ref["tail"][1] > 0
            assert (values == f32(3e38)).any()


BOXES = [
    ("window", None),
    ("both seams", ((5, 30, 35), (20, 15, 10))),            # y 30..45 and z 35..45 cross ring slot 40 -> 0
    ("odd x", ((3, 10, 12), (29, 7, 5))),
    ("odd x, one slot", ((1, 39, 39), (17, 3, 3))),
    ("partly outside", ((-5, 0, 40), (20, 20, 30))),
    ("outside", ((100, 100, 100), (4, 4, 4))),
    ("beyond int32", ((2**31 - 2, 8, 8), (2**31 - 1, 4, 4))),
    ("one voxel", ((17, 23, 41), (1, 1, 1))),
    ("empty shape", ((4, 10, 10), (0, 5, 5))),
]


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_boxes(kind):
    vol, rings = scene_of(kind)
    lo, hi = ranges_of(considered_texels(rings[0]))
    for name, box in BOXES:
        ref = histogram_twin(rings, 0, lo, hi, 256, box=box)
        same(c_hist(vol, 0, lo, hi, 256, box=box), ref, (kind, name))
        if name in ("outside", "beyond int32", "empty shape"):
            assert not ref["counts"].any() and not ref["tail"].any() and ref["range"].tolist() == [np.inf, -np.inf]
        elif name == "one voxel":
            assert ref["tail"][3] == 1
        else:
            assert ref["tail"][3] > 100
    same(c_hist(vol, 1, lo, hi, 64, box=((3, 2, 1), (21, 30, 31))), histogram_twin(rings, 1, lo, hi, 64, box=((3, 2, 1), (21, 30, 31))),
         (kind, "lod 1"))


def test_a_lod_without_a_window_counts_nothing():
    vol, rings = scene_of("u8")
    got = c_hist(vol, 2, 0.0, 256.0, 256)
    same(got, histogram_twin(rings, 2, 0.0, 256.0, 256), "lod 2")
    assert not got["counts"].any() and not got["tail"].any() and got["range"].tolist() == [np.inf, -np.inf]


def test_label_filter():
    vol, rings = scene_of("u8")
    ids, freq = np.unique(np.asarray(rings[0]["labels"]), return_counts=True)
    by_freq = ids[np.argsort(-freq)]
    absent = int(ids.max()) + 12345
    for lod in (0, 1):
        for labels in ([int(by_freq[0])], [int(v) for v in by_freq[1:4]], [absent], [absent, int(by_freq[2]), 0]):
            ref = histogram_twin(rings, lod, 0.0, 256.0, 256, labels=labels)
            same(c_hist(vol, lod, 0.0, 256.0, 256, labels=labels), ref, ("labels", lod, labels))
            assert ref["tail"][3] == 0 if labels == [absent] else ref["tail"][3] > 0
            res = vol.histogram(lod=lod, labels=labels[::-1] + labels)            # unsorted, repeated: sorted on the host
            assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), ref["counts"]) and res.considered == int(ref["tail"][3])
    box = ((3, 30, 35), (29, 15, 10))
    inside = [int(v) for v in by_freq if 0 < considered_texels(rings[0], box, [int(v)]).size < 29 * 15 * 10]
    ref = histogram_twin(rings, 0, 10.0, 200.0, 7, box=box, labels=inside[:1])
    same(c_hist(vol, 0, 10.0, 200.0, 7, box=box, labels=inside[:1]), ref, "labels in a box")
    assert 0 < ref["tail"][3] < 29 * 15 * 10


def test_label_filter_without_label_rings():
    vol, rings = scene_of("nolabels")
    assert not vol._rings.labels
    everything = histogram_twin(rings, 0, 0.0, 256.0, 256)
    same(c_hist(vol, 0, 0.0, 256.0, 256, labels=[0]), everything, "labels=[0]")
    same(c_hist(vol, 0, 0.0, 256.0, 256, labels=[0, 9]), everything, "labels=[0, 9]")
    nothing = c_hist(vol, 0, 0.0, 256.0, 256, labels=[5])
    same(nothing, histogram_twin(rings, 0, 0.0, 256.0, 256, labels=[5]), "labels=[5]")
    assert everything["tail"][3] == WINDOW0 and nothing["tail"][3] == 0 and not nothing["counts"].any()


def test_moving_window_and_constant_ring():
    """Three moves of the window, which wrap the rings on every axis: the histogram of every LOD equals the
    restatement's.  Then svr_clear_lod: the whole window sits in one bin (every lane of every wave on one counter)."""
    spec = spec_of("u8")
    vol = testing.build(spec).volume
    wrapped_x = False
    for position in ((20.0, 24.0, 30.0), (37.0, 33.0, 41.0), (44.5, 29.0, 35.0)):
        vol.center_on_position(position)
        spec.centers.append((position, None))
        rings = lmip.rings_of(lmip.oracle_volume(spec))
        wrapped_x |= bool(rings[0]["offset"][0] % 48)
        for lod in range(3):
            for bins, lo, hi in ((256, 0.0, 256.0), (7, 20.0, 130.0)):
                same(c_hist(vol, lod, lo, hi, bins), histogram_twin(rings, lod, lo, hi, bins), (position, lod, bins))
        box = ((int(rings[0]["offset"][0]) + 3, int(rings[0]["offset"][1]) + 1, int(rings[0]["offset"][2]) + 2), (37, 30, 33))
        same(c_hist(vol, 0, 0.0, 256.0, 256, box=box), histogram_twin(rings, 0, 0.0, 256.0, 256, box=box), (position, "box"))
    window = int(np.prod(rings[0]["shape"]))
    assert wrapped_x and window > 10000
    lib, handle = N.lib(), vol.prepare()
    N.check(lib.svr_clear_lod(handle, 0), "svr_clear_lod")
    N.check(lib.svr_publish_uploads(handle), "svr_publish_uploads")
    for bins, lo, hi, where in ((256, 0.0, 256.0, 0), (4096, -4095.5, 0.5, 4095), (1, -1.0, 1.0, 0)):
        got = c_hist(vol, 0, lo, hi, bins)
        assert got["counts"][where] == window and got["counts"].sum() == window, (bins, got["counts"].nonzero())
        assert got["tail"].tolist() == [0, 0, 0, window] and got["range"].tolist() == [0.0, 0.0]
    got = c_hist(vol, 0, 1.0, 2.0, 16)
    assert not got["counts"].any() and got["tail"].tolist() == [window, 0, 0, window]
    vol.close()


def test_micro_block_copy_does_not_change_the_counts():
    (with_copy, rings), (without, _) = scene_of("twin_all"), scene_of("twin_off")
    assert any(with_copy._rings.blocked_twin) and not any(without._rings.blocked_twin)
    ref = histogram_twin(rings, 0, 0.0, 256.0, 256)
    for lod in (0, 1):
        a, b = c_hist(with_copy, lod, 0.0, 256.0, 256), c_hist(without, lod, 0.0, 256.0, 256)
        same(a, b, ("copy", lod))
    same(c_hist(with_copy, 0, 0.0, 256.0, 256), ref, "copy against the restatement")


def test_renders_are_untouched():
    vol, _ = scene_of("u8")
    args = ((31.0, 30.0, 33.0), (0.5, 0.0, 0.0), (0.0, 0.4, 0.3), 96, 80)
    before = {k: getattr(vol.render_slice(*args), k).clone() for k in ("rgba", "value", "label", "flags", "lod")}
    vol.histogram(lod=0, bins=4096, labels=[117, 866, 5])
    vol.histogram(lod=1)
    after = vol.render_slice(*args)
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(t.view(torch.uint8), getattr(after, k).view(torch.uint8)), k
    assert int((after.flags == 2).sum()) > 100


def test_python_surface():
    vol, rings = scene_of("u8")
    res = vol.histogram()                                                      # lod 0, 256 bins over (0, 256)
    ref = histogram_twin(rings, 0, 0.0, 256.0, 256)
    assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), ref["counts"]) and res.lod == 0
    assert (res.under, res.over, res.nan, res.considered) == tuple(int(v) for v in ref["tail"])
    assert (res.min, res.max) == (float(ref["range"][0]), float(ref["range"][1]))
    assert np.array_equal(res.edges, edges_twin(0.0, 256.0, 256)) and res.counts.dtype == torch.int64 and res.counts.is_cuda
    # a box of the finest scale on LOD 1: floor(begin * 0.5), ceil(end * 0.5)
    begin, end = (9, 1, 3), (41, 63, 22)
    scale = vol.wrapping_buffers[1].scale_factor
    assert tuple(scale) == (0.5, 0.5, 0.5)
    res = vol.histogram(lod=1, bins=7, range=(20, 130), box=(begin, end))
    ref = histogram_twin(rings, 1, 20.0, 130.0, 7, box=lod_box_twin(begin, end, scale))
    assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), ref["counts"]) and res.considered == int(ref["tail"][3]) > 1000
    # auto_clim: the coarsest LOD that has a window (LOD 1), 256 bins on a byte ring; from the counts alone
    counts = histogram_twin(rings, 1, 0.0, 256.0, 256)["counts"]
    assert vol.auto_clim() == auto_clim_twin(counts, edges_twin(0.0, 256.0, 256))
    assert vol.auto_clim((2, 90), lod=0, bins=64, range=(10, 200)) == auto_clim_twin(
        histogram_twin(rings, 0, 10.0, 200.0, 64)["counts"], edges_twin(10.0, 200.0, 64), (2, 90))
    with pytest.raises(ValueError):
        vol.auto_clim(lod=2)                                                   # nothing resident: N == 0
    # a caller's stream: the id list is copied on torch's stream, the kernel runs on the other one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = vol.histogram(lod=0, labels=[866, 117], stream=side.cuda_stream)
    ref = histogram_twin(rings, 0, 0.0, 256.0, 256, labels=[117, 866])
    side.synchronize()
    assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), ref["counts"]) and res.considered == int(ref["tail"][3]) > 0
    assert res.selected.tolist() == [117, 866]
    # default ranges of the other storages
    vol16, rings16 = scene_of("u16")
    res = vol16.histogram(bins=4096)
    assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), histogram_twin(rings16, 0, 0.0, 65536.0, 4096)["counts"])
    assert res.edges[-1] == 65536.0
    volf, ringsf = scene_of("f32")
    with pytest.raises(ValueError):
        volf.histogram()                                                       # the seeded +-inf are the min and the max
    with pytest.raises(ValueError):
        volf.histogram(lod=2)                                                  # nothing resident
    # range=None on float32 rings: a first pass takes min and max, the histogram runs over [min, max].  The special
    # values sit in unlabelled voxels, so the labelled objects are finite
    labels = np.asarray(ringsf[0]["labels"])
    clean = [int(v) for v in np.unique(labels) if v != 0][:3]
    assert len(clean) == 3 and np.isfinite(considered_texels(ringsf[0], labels=clean)).all()
    for lod, box in ((0, None), (1, ((8, 2, 6), (60, 58, 64)))):
        twin_box = None if box is None else lod_box_twin(*box, volf.wrapping_buffers[lod].scale_factor)
        values = considered_texels(ringsf[lod], twin_box, clean)
        assert values.size > 1000 and float(values.min()) < 0.0 < float(values.max())
        res = volf.histogram(lod=lod, bins=100, labels=clean, box=box)
        assert (res.min, res.max) == (float(values.min()), float(values.max()))
        ref = histogram_twin(ringsf, lod, res.min, res.max, 100, box=twin_box, labels=clean)
        assert np.array_equal(res.counts.cpu().numpy().view(np.uint64), ref["counts"])
        assert (res.under, res.over, res.nan, res.considered) == (0, 0, 0, values.size)
        assert ref["counts"][99] > 0 and ref["counts"][0] > 0                   # the closed top bin holds the maximum
        assert np.array_equal(res.edges, edges_twin(res.min, res.max, 100)) and res.edges[0] == res.min and res.edges[-1] == res.max
    low, high = volf.auto_clim(labels=clean)                                   # LOD 1, 4096 bins over its [min, max]
    values = considered_texels(ringsf[1], labels=clean)
    lo1, hi1 = float(values.min()), float(values.max())
    assert (low, high) == auto_clim_twin(histogram_twin(ringsf, 1, lo1, hi1, 4096, labels=clean)["counts"], edges_twin(lo1, hi1, 4096))
    with pytest.raises(ValueError):
        volf.histogram(box=((20, 20, 20), (21, 21, 21)))                       # one voxel: min == max


def test_refusals_enqueue_nothing():
    vol, rings = scene_of("u8")
    lib, handle = N.lib(), vol.prepare()
    dev = torch.device("cuda", vol._rings.device)
    present = np.unique(np.asarray(rings[0]["labels"]))
    counts = torch.full((4096,), -7, dtype=torch.int64, device=dev)
    tail = torch.full((4,), -7, dtype=torch.int64, device=dev)
    rng = torch.full((2,), 7.0, dtype=torch.float32, device=dev)
    sel = torch.tensor([int(present[1]), int(present[2])], dtype=torch.int32, device=dev)
    inf, nan = float("inf"), float("nan")

    def params(**kw):
        hp = N.HistogramParams(lod=0, lo=0.0, hi=256.0, bins=256)
        for k, v in kw.items():
            if k in ("box_off", "box_shape"):
                getattr(hp, k)[:] = v
            else:
                setattr(hp, k, v)
        return hp

    def call(hp=None, h=handle, null=(), no_counts=False):
        hp = hp or params()
        ho = N.HistogramOutputs(None if no_counts else counts.data_ptr(), tail.data_ptr(), rng.data_ptr())
        return lib.svr_histogram(h, None if "params" in null else C.byref(hp), None if "out" in null else C.byref(ho), None)

    cases = [
        (dict(h=None), "null argument"), (dict(null=("params",)), "null argument"), (dict(null=("out",)), "null argument"),
        (dict(no_counts=True), "null argument"),
        (dict(hp=params(lod=-1)), "lod out of range"), (dict(hp=params(lod=3)), "lod out of range"),
        (dict(hp=params(bins=0)), "bins must be in"), (dict(hp=params(bins=4097)), "bins must be in"),
        (dict(hp=params(lo=nan)), "lo and hi must be finite"), (dict(hp=params(hi=inf)), "lo and hi must be finite"),
        (dict(hp=params(lo=-inf)), "lo and hi must be finite"), (dict(hp=params(lo=256.0)), "lo and hi must be finite"),
        (dict(hp=params(lo=300.0)), "lo and hi must be finite"),
        (dict(hp=params(lo=0.0, hi=1e-38, bins=4096)), "not finite in f32"),
        (dict(hp=params(use_box=1, box_off=(0, 8, 8), box_shape=(4, -1, 4))), "negative box_shape"),
        (dict(hp=params(selected=None, selected_count=2)), "NULL selected"),
    ]
    for kw, msg in cases:
        assert call(**kw) == -1, (kw, msg)
        assert msg in lib.svr_last_error().decode(), (msg, lib.svr_last_error())
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((tail == -7).all()) and bool((rng == 7.0).all())      # nothing was enqueued
    # the control cases run: with an id list, and with only the counts wanted
    assert call(params(selected=sel.data_ptr(), selected_count=2)) == 0
    torch.cuda.synchronize()
    assert int(tail[3]) == int(counts[:256].sum()) > 0 and bool((counts[256:] == -7).all()) and float(rng[0]) <= float(rng[1])
    only = torch.full((256,), -7, dtype=torch.int64, device=dev)
    ho = N.HistogramOutputs(only.data_ptr(), None, None)
    assert lib.svr_histogram(handle, C.byref(params()), C.byref(ho), None) == 0
    torch.cuda.synchronize()
    assert int(only.sum()) == WINDOW0
