"""No GPU: the numpy restatement of svr_histogram (tests/histogram_twin.py) against numpy's own histograms where the
two must agree, its tails, the arithmetic of ``auto_clim``, the box -> LOD mapping, the windows the GPU tests rely on,
and the refusals the Python surface makes before it touches the device."""
import numpy as np
import pytest

from histogram_twin import (auto_clim_twin, bin_values, considered_texels, edges_twin, histogram_twin, lod_box_twin)
from oracle import lmip
from sub_volume_renderer_amd import HistogramResult, SubVolume, SubVolumeMaterial, _native as N, testing
from sub_volume_renderer_amd._wobject import clim_from_counts, histogram_edges, label_ids, lod_box

f32 = np.float32


def test_integer_data_over_0_256_is_bincount():
    rng = np.random.default_rng(1)
    v = rng.integers(0, 256, 5000).astype(np.uint8)
    got = bin_values(v, 0, 256, 256)
    assert np.array_equal(got["counts"], np.bincount(v, minlength=256))
    assert got["tail"].tolist() == [0, 0, 0, 5000] and got["range"].tolist() == [float(v.min()), float(v.max())]
    v16 = (rng.integers(0, 256, 5000) * 251).astype(np.uint16)
    got = bin_values(v16, 0, 65536, 4096)
    assert np.array_equal(got["counts"], np.bincount(v16 // 16, minlength=4096))


def test_equals_numpy_histogram_where_the_chain_is_exact():
    """Dyadic values and power-of-two bin widths: v - lo and (v - lo) * inv are exact in f32 and in float64."""
    rng = np.random.default_rng(2)
    v = (rng.integers(-64, 192, 4000) / 8.0).astype(f32)              # multiples of 1/8 in [-8, 24)
    for lo, hi, k in ((-8.0, 24.0, 256), (-8.0, 24.0, 32), (0.0, 16.0, 64), (-4.0, 4.0, 1)):
        got = bin_values(v, lo, hi, k)
        ref, _ = np.histogram(v.astype(np.float64), bins=k, range=(lo, hi))
        assert np.array_equal(got["counts"], ref), (lo, hi, k)
        assert int(got["tail"][0]) == int((v < lo).sum()) and int(got["tail"][1]) == int((v > hi).sum())


def test_hi_is_closed_and_the_tails_take_the_rest():
    v = np.array([10.0, 9.999, 0.0, -0.0, -1e-3, 10.001, np.nan, np.inf, -np.inf, -5.0, 5.0], f32)
    got = bin_values(v, 0.0, 10.0, 7)
    assert got["counts"][6] == 2 and got["counts"][0] == 2 and got["counts"][3] == 1 and got["counts"].sum() == 5
    assert got["tail"].tolist() == [3, 2, 1, 11]                        # under: -1e-3, -inf, -5; over: 10.001, +inf
    assert got["range"][0] == -np.inf and got["range"][1] == np.inf     # the range covers under and over, never NaN
    only_nan = bin_values(np.array([np.nan, np.nan], f32), 0.0, 1.0, 4)
    assert only_nan["tail"].tolist() == [0, 0, 2, 2] and only_nan["range"].tolist() == [np.inf, -np.inf]
    nothing = bin_values(np.zeros(0, f32), 0.0, 1.0, 4)
    assert not nothing["counts"].any() and not nothing["tail"].any() and nothing["range"].tolist() == [np.inf, -np.inf]
    one_bin = bin_values(v, 0.0, 10.0, 1)
    assert one_bin["counts"].tolist() == [5]


def test_a_range_wider_than_f32_puts_everything_in_bin_0():
    """hi - lo overflows to inf, inv == 0: every product is 0, or NaN where v - lo overflows too; both are bin 0."""
    v = np.array([3e38, -3e38, 0.0, 1e30, np.inf, -np.inf, np.nan, 3.4e38], f32)
    for k in (1, 4, 4096):
        got = bin_values(v, -3e38, 3e38, k)
        assert got["counts"][0] == 4 and got["counts"].sum() == 4 and got["tail"].tolist() == [1, 2, 1, 8]


def ring_of(density, offset, shape, labels=None):
    return dict(density=density, labels=labels, offset=offset, shape=shape, scale=(1.0, 1.0, 1.0))


def test_window_wrap_box_and_label_filter():
    rng = np.random.default_rng(3)
    density = rng.integers(0, 256, (6, 5, 8)).astype(np.uint8)          # ring [z][y][x] = 8 x 5 x 6 slots
    labels = rng.integers(0, 4, (6, 5, 8)).astype(np.uint32)
    ring = ring_of(density, offset=(6, 3, 10), shape=(8, 4, 5), labels=labels)      # wraps on every axis
    whole = considered_texels(ring)
    zs, ys, xs = np.arange(10, 15) % 6, np.arange(3, 7) % 5, np.arange(6, 14) % 8
    assert np.array_equal(whole, density[np.ix_(zs, ys, xs)].astype(f32).reshape(-1))
    part = considered_texels(ring, box=((4, 5, 12), (5, 9, 1)))          # x 6..8, y 5..6, z 12
    assert np.array_equal(part, density[np.ix_([12 % 6], [0, 1], [6, 7, 0])].astype(f32).reshape(-1))
    assert considered_texels(ring, box=((14, 3, 10), (4, 4, 4))).size == 0              # misses the window
    assert considered_texels(ring_of(density, (0, 0, 0), (0, 0, 0))).size == 0         # a window of None
    kept = considered_texels(ring, labels=[1, 3])
    sel = np.isin(labels[np.ix_(zs, ys, xs)].reshape(-1), [1, 3])
    assert np.array_equal(kept, whole[sel]) and 0 < kept.size < whole.size
    # no label ring: every label reads as 0
    assert considered_texels(ring_of(density, (6, 3, 10), (8, 4, 5)), labels=[0]).size == whole.size
    assert considered_texels(ring_of(density, (6, 3, 10), (8, 4, 5)), labels=[5]).size == 0
    h = histogram_twin([ring], 0, 0, 256, 256, labels=[1, 3])
    assert np.array_equal(h["counts"], np.bincount(kept.astype(np.int64), minlength=256))


def test_the_windows_the_gpu_tests_rely_on():
    spec = testing.synthetic_spec(64, 96, 80)
    rings = lmip.rings_of(lmip.oracle_volume(spec))
    assert tuple(rings[0]["offset"]) == (0, 8, 8) and tuple(rings[0]["shape"]) == (48, 40, 40)
    assert rings[0]["density"].shape == (40, 40, 48)                      # the window fills the ring and wraps in y, z
    assert tuple(rings[1]["shape"]) == (32, 32, 32) and rings[1]["density"].shape == (32, 32, 32)
    assert all(o % 32 == 0 for o in rings[1]["offset"])                   # unwrapped
    assert tuple(rings[2]["shape"]) == (0, 0, 0)                          # no window
    assert len(np.unique(considered_texels(rings[0]))) > 16


def test_auto_clim_arithmetic():
    edges = histogram_edges(0.0, 256.0, 256)
    assert np.array_equal(edges, np.arange(257.0)) and np.array_equal(edges, edges_twin(0.0, 256.0, 256))
    spike = np.zeros(256); spike[40] = 1000
    assert clim_from_counts(spike, edges) == (40.0, 41.0) == auto_clim_twin(spike, edges)
    two = np.zeros(256); two[10] = 500; two[200] = 500
    assert clim_from_counts(two, edges) == (10.0, 201.0) == auto_clim_twin(two, edges)
    assert clim_from_counts(two, edges, (50.0, 50.0)) == auto_clim_twin(two, edges, (50.0, 50.0))      # c_j meets the target
    assert clim_from_counts(two, edges, (50.0, 100.0)) == (200.0, 201.0)                               # strictly above the low one
    ramp = np.arange(256.0)
    ramp[:3] = 0; ramp[250:] = 0
    assert clim_from_counts(ramp, edges, (0, 100)) == (3.0, 250.0) == auto_clim_twin(ramp, edges, (0, 100))
    rng = np.random.default_rng(4)
    for _ in range(20):
        k = int(rng.integers(1, 300))
        counts = rng.integers(0, 50, k) * (rng.random(k) < 0.4)
        if not counts.any():
            continue
        e = histogram_edges(-3.5, 17.25, k)
        p = sorted(rng.uniform(0, 100, 2))
        assert clim_from_counts(counts, e, p) == auto_clim_twin(counts, e, p)
    with pytest.raises(ValueError):
        clim_from_counts(np.zeros(16), histogram_edges(0, 1, 16))         # N == 0
    for bad in ((60, 40), (-1, 50), (0, 101), (1,), "ab"):
        with pytest.raises(ValueError):
            clim_from_counts(spike, edges, bad)


def test_box_to_lod_mapping():
    assert lod_box((8, 0, 3), (40, 17, 21), (1.0, 1.0, 1.0)) == ((8, 0, 3), (40, 17, 21))
    assert lod_box((9, 1, 3), (41, 17, 22), (0.5, 0.5, 0.5)) == ((4, 0, 1), (21, 9, 11))          # floor begin, ceil end
    assert lod_box((9, 1, 3), (10, 2, 4), (0.25, 0.25, 1.0)) == ((2, 0, 3), (3, 1, 4))
    assert lod_box((-3, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5)) == ((-2, 0, 0), (1, 1, 1))
    for begin, end, scale in (((9, 1, 3), (41, 17, 22), (0.5, 0.5, 0.25)), ((0.5, 2.5, 7), (3.25, 2.75, 8), (0.5, 1.0, 0.125))):
        b, e = lod_box(begin, end, scale)
        assert lod_box_twin(begin, end, scale) == (b[::-1], tuple(ev - bv for bv, ev in zip(b[::-1], e[::-1])))
    for bad in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 0, 1)), ((0, 0, np.nan), (1, 1, 1)), ((0, 0, 0), (1, 1, 1e12))):
        with pytest.raises(ValueError):
            lod_box(*bad, (1.0, 1.0, 1.0))


def test_label_ids_are_sorted_and_unique():
    assert label_ids([7, 3, 7, 2**32 - 1, 0]).tolist() == [0, 3, 7, 2**32 - 1]
    assert label_ids(np.array([5, 5], np.uint32)).dtype == np.uint32
    for bad in ([], [-1], [2**32], [1.5], [True], "12", 7):
        with pytest.raises(ValueError):
            label_ids(bad)


def test_python_refusals_come_before_the_device(monkeypatch):
    """Every refusal is raised from the arguments alone: ``prepare`` (the first device use) is never reached."""
    d = [np.zeros((16 >> k,) * 3, np.uint8) for k in range(2)]
    vol = SubVolume(SubVolumeMaterial(0.5), [(d[0], d[0]), (d[1], d[1])], (2, 2, 2), (4, 4, 4))

    def no_device():
        raise AssertionError("the device was reached")

    monkeypatch.setattr(vol, "prepare", no_device)
    bad = [dict(lod=2), dict(lod=-1), dict(lod=0.0), dict(lod=True), dict(bins=0), dict(bins=N.HIST_MAX_BINS + 1),
           dict(bins=16.0), dict(range=(1.0, 1.0)), dict(range=(2.0, 1.0)), dict(range=(0.0, float("inf"))),
           dict(range=(float("nan"), 1.0)), dict(range=(0.0, 1e39)), dict(range=(0.0,)), dict(range="ab"),
           dict(box=((0, 0, 0),)), dict(box=((0, 0, 0), (0, 4, 4))), dict(box=((0, 0), (4, 4, 4))), dict(box=7),
           dict(labels=[]), dict(labels=[-1]), dict(labels=[1.5]), dict(labels="3")]
    for kw in bad:
        with pytest.raises(ValueError):
            vol.histogram(**kw)
    for kw in (dict(percentiles=(60, 40)), dict(percentiles=(0, 101)), dict(percentiles=(1,)), dict(lod=5), dict(bins=0)):
        with pytest.raises(ValueError):
            vol.auto_clim(**kw)
    with pytest.raises(ValueError):
        vol.auto_clim()                                                   # no LOD has a window yet
    with pytest.raises(AssertionError):
        vol.histogram()                                                   # the control case gets as far as the device
    assert {"counts", "tail", "range", "edges", "lod"} <= set(HistogramResult.__dataclass_fields__)
    assert N.HistogramParams.bins.offset == 40 and N.HistogramParams.selected.offset == 48      # the C layout
