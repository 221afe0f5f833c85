"""render_slice's host checks work in float32, the precision of the kernel: vectors that are finite in float64 but
overflow float32, and u / v that are parallel once rounded to float32, are refused before any device work; a string
is not a vector."""
import numpy as np
import pytest

from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial


def small_volume():
    d = np.zeros((16, 16, 16), np.uint8)
    return SubVolume(SubVolumeMaterial(0.5), [(d, d)], (2, 2, 2), (4, 4, 4))


def test_vectors_are_checked_in_float32_before_device_work(monkeypatch):
    vol = small_volume()
    touched = []
    monkeypatch.setattr(vol, "prepare", lambda: touched.append(1))
    ok = dict(origin=(0, 0, 0), u=(1, 0, 0), v=(0, 1, 0), width=8, height=6)
    cases = [
        (dict(origin="123"), "origin must be three finite numbers"),
        (dict(u=b"abc"), "u must be three finite numbers"),
        (dict(origin=(0.0, 1e39, 0.0)), "origin must be three numbers that are finite in float32"),
        (dict(u=(1.0, 0.0, -4e38)), "u must be three numbers that are finite in float32"),
        (dict(v=(3.5e38, 3.5e38, 0.0)), "v must be three numbers that are finite in float32"),
        # nonzero in float64, 0 once the float32 products underflow: no plane for the kernel
        (dict(u=(1e-30, 0.0, 0.0), v=(0.0, 1e-30, 0.0)), "u and v must be nonzero and not parallel"),
        # not parallel in float64, parallel once rounded to float32
        (dict(u=(1.0, 1.0 + 1e-12, 0.0), v=(1.0, 1.0, 0.0)), "u and v must be nonzero and not parallel"),
    ]
    for bad, msg in cases:
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError) as e:
            vol.render_slice(**kw)
        assert msg in str(e.value), (bad, str(e.value))
    assert not touched
    with pytest.raises(ValueError):
        SubVolume.axis_slice_plane("z", "123")
    with pytest.raises(ValueError):
        SubVolume.axis_slice_plane("z", (0, 0, 0), 1e39)
