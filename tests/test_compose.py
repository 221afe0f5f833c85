"""Display-side compose: numpy restatement properties on CPU, HIP kernel vs the
restatement on the GPU.  Blending / encode are pygfx behaviour restated: parity unpinned."""
import math

import numpy as np
import pytest

import compose_f64 as F
from oracle import compose_oracle, lmip
from sub_volume_renderer_amd import testing


def test_oracle_known_values():
    rgba = np.zeros((2, 3, 4), np.float32)
    rgba[0, 0] = (1.0, 0.5, 0.0, 1.0)          # opaque fragment
    rgba[0, 1] = (1.0, 1.0, 1.0, 0.5)          # half-transparent white
    flags = np.array([[2, 1, 0], [0, 0, 0]], np.uint8)
    q, _ = compose_oracle.compose(rgba, flags=flags, bg_bottom=(0, 0, 0, 1), bg_top=(0, 0, 0, 1))
    assert tuple(q[0, 0]) == (255, 188, 0, 255)                      # sRGB(0.5) = 0.7354 -> 188
    assert tuple(q[0, 1]) == (188, 188, 188, 255)                    # 0.5 over black, alpha 0.5 + 1*0.5
    assert tuple(q[0, 2]) == (0, 0, 0, 255) and tuple(q[1, 1]) == (0, 0, 0, 255)   # discarded: background
    # gradient: top row nearer bg_top
    q2, _ = compose_oracle.compose(np.zeros((4, 1, 4), np.float32), flags=np.zeros((4, 1), np.uint8),
                                   bg_bottom=(1, 1, 1, 1), bg_top=(0, 0, 0, 1), srgb=False)
    assert list(q2[:, 0, 0]) == [32, 96, 159, 223]
    # depth test keeps what is nearer
    z = np.array([[0.2, 0.9]], np.float32)
    d = np.array([[0.5, 0.5]], np.float32)
    px = np.ones((1, 2, 4), np.float32)
    q3, z3 = compose_oracle.compose(px, depth=d, zbuf=z, srgb=False)
    assert tuple(q3[0, 0]) == (0, 0, 0, 255) and tuple(q3[0, 1]) == (255, 255, 255, 255)
    np.testing.assert_array_equal(z3, np.array([[0.2, 0.5]], np.float32))


def _grey(c):
    """A 1 x 1 opaque grey of float32 value c over black: the blend is c * 1 + 0 * 0 = c exactly."""
    return np.array([[[c, c, c, 1.0]]], np.float32)


def test_float64_reference_known_values():
    f = lambda x: float(np.float32(x))                                                  # noqa: E731
    v, draw = F.reference(np.array([[[1.0, 0.5, 0.0, 1.0]]], np.float32))
    assert draw.all() and F.decidable(v).all()
    assert tuple(F.levels(v)[0, 0]) == (255, 188, 0, 255)                               # sRGB(0.5) = 0.7354 -> 188.03
    assert abs(v[0, 0, 1] - ((f(1.055) * 0.5 ** f(np.float32(1) / np.float32(2.4)) - f(0.055)) * 255 + 0.5)) < 1e-9
    # the knee: 0.0031308f itself and the value below it take the linear branch, the one above it the power branch;
    # the two branches meet there within 2e-5 levels, far below DELTA, so the side a float32 blend lands on is not seen
    knee = np.float32(0.0031308)
    below, above = np.nextafter(knee, np.float32(0)), np.nextafter(knee, np.float32(1))
    for c in (below, knee):
        v, _ = F.reference(_grey(c))
        assert abs(v[0, 0, 0] - (f(12.92) * float(c) * 255 + 0.5)) < 1e-12 and F.levels(v)[0, 0, 0] == 10   # 10.81
    v, _ = F.reference(_grey(above))
    power = lambda c: (f(1.055) * math.pow(float(c), f(np.float32(1) / np.float32(2.4))) - f(0.055)) * 255 + 0.5   # noqa: E731
    assert abs(v[0, 0, 0] - power(above)) < 1e-9 and F.levels(v)[0, 0, 0] == 10
    assert abs(power(knee) - (f(12.92) * float(knee) * 255 + 0.5)) < 2e-5
    # 0 -> 0 and 1 -> 255 (1.055f - 0.055f is a little under 1: v = 255.49998..)
    v, _ = F.reference(_grey(0.0))
    assert v[0, 0, 0] == 0.5 and F.levels(v)[0, 0, 0] == 0
    v, _ = F.reference(_grey(1.0))
    assert 255.499 < v[0, 0, 0] <= 255.5 and tuple(F.levels(v)[0, 0]) == (255, 255, 255, 255)
    # the four-row gradient: t = 1/8, 3/8, 5/8, 7/8 exactly, v = 255 t + 0.5
    v, draw = F.reference(np.zeros((4, 1, 4), np.float32), flags=np.zeros((4, 1), np.uint8), bg_bottom=(1, 1, 1, 1),
                          bg_top=(0, 0, 0, 1), srgb=False)
    assert not draw.any()
    assert list(v[:, 0, 0]) == [32.375, 96.125, 159.875, 223.625] and list(F.levels(v)[:, 0, 0]) == [32, 96, 159, 223]
    # a discarded pixel and a fragment behind the canvas both show the background; NaN clamps to 0
    v, draw = F.reference(np.ones((1, 3, 4), np.float32) * np.array([1, 1, 1, 1], np.float32), depth=np.array([[0.5, 0.5, np.nan]], np.float32),
                          zbuf=np.array([[0.9, 0.5, 0.9]], np.float32), srgb=False)
    assert draw.tolist() == [[True, False, False]] and list(F.levels(v)[0, :, 0]) == [255, 0, 0]
    v, _ = F.reference(np.array([[[np.nan, np.inf, -np.inf, 1.0]]], np.float32))
    assert tuple(F.levels(v)[0, 0]) == (0, 255, 0, 255)


_FAMILY_CASES = [(fam, combo) for fam in F.FAMILIES for combo in F.COMBOS] + [(F.BIG, F.COMBOS[2])]


@pytest.mark.parametrize("family,combo", _FAMILY_CASES, ids=[f"{f[0]}-{c[0]}" for f, c in _FAMILY_CASES])
def test_oracle_equals_float64_reference_on_the_gpu_families(family, combo):
    """The float32 restatement against the float64 one on the inputs of test_gpu_compose.py: floor(v) on every decidable
    value, one level at most on the rest; which pixels are drawn and the depth plane agree exactly.  And the condition
    of the GPU comparison, from the float64 reference alone: at most 1 % of a channel's values are undecidable (frames
    of fewer than 100 values: none)."""
    _, seed, h, w, (bottom, top) = family
    p = F.planes(seed, h, w)
    kw = F.combo_args(p, combo)
    for srgb in (False, True):
        q, z = compose_oracle.compose(p["rgba"], bg_bottom=bottom, bg_top=top, srgb=srgb, **kw)
        v, draw = F.reference(p["rgba"], bg_bottom=bottom, bg_top=top, srgb=srgb, **kw)
        F.hold(q, v, (family[0], combo[0], srgb))
        share = (~F.decidable(v)).mean(axis=(0, 1))
        assert (share <= 0.01).all(), (family[0], combo[0], srgb, share)
        if kw["zbuf"] is not None:
            np.testing.assert_array_equal(z.view(np.uint32), np.where(draw, p["depth"], p["zbuf"]).view(np.uint32))
            assert 0 < draw.sum() < draw.size or draw.size == 1


def test_oracle_nan_rule():
    """include/svr.h: the clamps are fminf(fmaxf(v, 0), 1), so a NaN channel quantises to 0; a NaN depth fails "<"."""
    nan, inf = np.nan, np.inf
    rgba = np.array([[[nan, 0.5, nan, 1.0],            # NaN rgb under an opaque alpha
                      [0.5, 0.5, 0.5, nan],            # NaN alpha poisons all four channels
                      [1.0, 1.0, 1.0, 1.0],            # NaN depth: not drawn
                      [inf, -inf, 0.5, 1.0]]], np.float32)
    depth = np.array([[0.1, 0.1, nan, 0.1]], np.float32)
    zbuf = np.array([[0.5, 0.5, 0.5, 0.5]], np.float32)
    bg = (0.2, 0.4, 0.6, 1.0)                          # 0.2f * 255 + 0.5 = 51.5, 102.5, 153.5: nowhere near a floor
    q, z = compose_oracle.compose(rgba, depth=depth, zbuf=zbuf, bg_bottom=bg, bg_top=bg, srgb=False)
    assert q.tolist() == [[[0, 128, 0, 255], [0, 0, 0, 0], [51, 102, 153, 255], [255, 0, 128, 255]]]
    np.testing.assert_array_equal(z, np.array([[0.1, 0.1, 0.5, 0.1]], np.float32))
    q, _ = compose_oracle.compose(rgba, depth=depth, zbuf=zbuf, bg_bottom=(0, 0, 0, 1), bg_top=(0, 0, 0, 1), srgb=True)
    assert q.tolist() == [[[0, 188, 0, 255], [0, 0, 0, 0], [0, 0, 0, 255], [255, 0, 188, 255]]]
    q, z = compose_oracle.compose(rgba, depth=depth, zbuf=np.full((1, 4), nan, np.float32), srgb=False)
    assert q.tolist() == [[[0, 0, 0, 255]] * 4] and np.isnan(z).all()              # a NaN on the canvas side fails "<" too
    v, draw = F.reference(rgba, depth=depth, zbuf=zbuf, bg_bottom=bg, bg_top=bg, srgb=False)
    assert draw.tolist() == [[True, True, False, True]]
    assert F.levels(v).tolist() == [[[0, 128, 0, 255], [0, 0, 0, 0], [51, 102, 153, 255], [255, 0, 128, 255]]]


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [False, True])
def test_compose_kernel_matches_restatement(with_depth):
    import torch

    from sub_volume_renderer_amd.compose import compose

    spec = testing.synthetic_spec(64, 150, 90, threshold=0.4)
    spec.material["opacity"] = 0.8
    scene = testing.build(spec)
    res = scene.volume.render(scene.camera, scene.width, scene.height)
    torch.cuda.synchronize()
    bottom, top = (100 / 255, 100 / 255, 100 / 255, 1.0), (169 / 255, 167 / 255, 168 / 255, 1.0)   # tests/conftest.py:18-19
    rng = np.random.default_rng(5)
    z0 = rng.random((scene.height, scene.width), dtype=np.float32) if with_depth else None
    zdev = torch.from_numpy(z0.copy()).to(res.rgba.device) if with_depth else None
    got = compose(scene.volume, res, background=(bottom, top), depth_buffer=zdev)
    torch.cuda.synchronize()
    want, zwant = compose_oracle.compose(res.rgba.cpu().numpy(), res.depth.cpu().numpy(), res.flags.cpu().numpy(),
                                         bottom, top, zbuf=z0)
    diff = np.abs(got.cpu().numpy().astype(np.int16) - want.astype(np.int16))
    assert diff.max() <= 1, diff.max()                                 # powf: 1 LSB at most
    assert (diff > 0).mean() < 0.01
    assert (res.flags == 2).sum().item() > 100
    if with_depth:
        np.testing.assert_array_equal(zdev.cpu().numpy(), zwant)
        assert 0 < (zwant != z0).sum() < z0.size                       # some fragments passed, some did not
    # the render itself agrees with the oracle (so the composed image is the oracle's, composed)
    ref = lmip.render_spec(spec)
    assert np.array_equal(res.flags.cpu().numpy(), ref.flags)
