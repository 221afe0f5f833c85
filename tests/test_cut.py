"""CPU: the cut planes' restatement (tests/cut_twin.py) against answers that do not come from it - caps of a solid cube
at the plane with the plane's normal and a Blinn-Phong colour computed by hand, the monotonicity the kernels build
their index interval on, planes that cut nothing / everything, a composite ray with its middle removed - and the
Python surface: the material's ``cut_planes`` / ``cut_mode``, ``SubVolume.crop_planes``, the refusal of the march
modes, and svr_set_cut_planes in header, binding and library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import composite_twin
import cut_twin
import iso_twin
import linear_twin
from slice_twin import DISCARD, HIT, MISS
from sub_volume_renderer_amd import SubVolume, SubVolumeMaterial, _native
from sub_volume_renderer_amd._transform import AffineTransform
from test_iso import FRAME, N, NSTEPS, SHADE, material, ring, spec_for, step_along_x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZE = (f32(N),) * 3
SOLID = np.full((N, N, N), 200, np.uint8)


def iso(rings, M, planes, mode="ANY", linear=False, **params):
    p = dict(SHADE)
    p.update(params)
    return iso_twin.iso_twin(rings, M, SIZE, material(), FRAME, FRAME, p, pick_id=5, cut_planes=planes, cut_mode=mode,
                             linear=linear)


def tilted_world():
    """The block rotated and anisotropically scaled about its centre."""
    t = AffineTransform()
    q = np.array([0.1, -0.15, 0.05, 0.0])
    q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    t.set_rotation_quaternion(q)
    t.scale = (1.1, 0.9, 1.05)
    c = np.full(3, (N - 1) / 2.0)
    t.position = tuple(c - t.matrix[:3, :3] @ c)
    return t


def matrices(spec, world=None):
    M = spec.matrices()
    if world is not None:
        M["world"], M["world_inv"] = np.asarray(world.matrix, f32), np.asarray(world.inverse_matrix, f32)
    return M


def predicate64(M, planes, S):
    """E_k per sample in float64, from world points: [K][rays, samples] for the rays of a set-up."""
    W = np.asarray(M["world"], np.float64)
    out = []
    n = int(S["nsteps"].max())
    i = np.arange(n, dtype=np.float64)
    p = [(S["start"][a].astype(np.float64) * N - 0.5)[..., None] + i * (S["step"][a].astype(np.float64) * N)[..., None]
         for a in range(3)]
    w = [W[r, 0] * p[0] + W[r, 1] * p[1] + W[r, 2] * p[2] + W[r, 3] for r in range(3)]
    for a, b, c, d in planes:
        out.append(a * w[0] + b * w[1] + c * w[2] - d)
    return out


# ---- 1, 2: caps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 4, 16])
def test_a_plane_across_a_solid_cube_gives_caps_at_the_plane(refine):
    spec = spec_for("+x")
    d = 12.3                                                 # world x of the plane: what lies at x < 12.3 is cut away
    out = iso([ring(SOLID)], matrices(spec), [(2.0, 0.0, 0.0, 2.0 * d)], iso_value=100.0, refine=refine)
    assert (out["flags"] == HIT).all() and (out["cap"] == 0).all()
    # sample i sits at the data coordinate i * 32 / 113, i.e. at world x = i * 32 / 113 - 0.5
    x = out["iter"].astype(np.float64) * N / NSTEPS - 0.5
    sub = N / NSTEPS / max(refine, 1)
    assert (x >= d).all() and (x - d < sub).all(), (x.min(), x.max())
    uncut = iso([ring(SOLID)], matrices(spec), [], iso_value=100.0, refine=refine)
    assert (uncut["iter"] == 0.0).all() and (uncut["cap"] == -1).all()
    # the plane's unit normal (1, 0, 0), turned to face the viewer: v = (-1, 0, 0)
    assert np.array_equal(out["normal"], np.broadcast_to(np.array([-1.0, 0.0, 0.0], f32), (FRAME, FRAME, 3)))
    # n = v = l = h: |n.l| = |n.h| = 1, so rgb = base * (ambient + diffuse) + specular exactly
    assert np.array_equal(out["rgba"], np.broadcast_to(np.array([0.5 * 0.75 + 0.125, 0.75 + 0.125, 0.25 * 0.75 + 0.125, 0.75], f32),
                                                       (FRAME, FRAME, 4)))
    first = math.ceil((d + 0.5) * NSTEPS / N)                # the first coarse sample in front of the plane: 46
    assert np.array_equal(out["steps"], np.full((FRAME, FRAME), first + 1, np.uint32))
    # seen at an angle the cap shades with the cosine: v = l = h = (-0.6, -0.8, 0)
    from test_iso import angled
    out = iso([ring(SOLID)], matrices(spec_for(angled)), [(1.0, 0.0, 0.0, d)], iso_value=100.0, refine=refine)
    caps = out["cap"] == 0
    assert caps.sum() > 60
    assert np.array_equal(out["normal"][caps], np.broadcast_to(np.array([-1.0, 0.0, 0.0], f32), (int(caps.sum()), 3)))
    t, s = 0.25 + 0.5 * 0.6, 0.125 * 0.6 ** 4
    assert np.abs(out["rgba"][caps] - np.array([0.5 * t + s, t + s, 0.25 * t + s, 0.75])).max() < 2e-6


@pytest.mark.parametrize("mode", ["ANY", "ALL"])
def test_an_oblique_plane_under_a_tilted_world_caps_with_nhat(mode):
    spec = spec_for("+x")
    world = tilted_world()
    M = matrices(spec, world)
    n = np.array([0.8, -0.36, -0.48])
    c = np.full(3, (N - 1) / 2.0)
    plane = tuple(3.0 * n) + (3.0 * float(n @ c) + 0.7,)     # not normalised: nhat is
    refine = 4
    out = iso([ring(SOLID)], M, [plane], mode, iso_value=100.0, refine=refine)
    caps = out["cap"] == 0
    assert (out["flags"] == HIT).all() and caps.sum() > 200
    S = iso_twin.setup_rays(M, SIZE, material(), FRAME, FRAME, None)
    E = predicate64(M, [plane], S)[0]
    it = out["iter"].astype(np.float64)
    lo = np.floor(it).astype(int)
    e_hit = np.take_along_axis(E, lo[..., None], -1)[..., 0] + (it - lo) * (E[..., 1] - E[..., 0])
    per_sub = np.abs(E[..., 1] - E[..., 0]) / refine
    assert (e_hit[caps] > -1e-3).all() and (e_hit[caps] < per_sub[caps] + 1e-3).all()
    # the rays travel along +x, so the viewer is towards -x: nhat faces it as it is when its x is negative
    want = -n if n[0] > 0 else n
    assert np.abs(out["normal"][caps] - want).max() < 1e-6
    # ... and that is not the gradient's answer: inside a constant block the gradient is zero and n would be v
    uncut = iso([ring(SOLID)], M, [], mode, iso_value=100.0, refine=refine)
    assert np.abs(uncut["normal"][caps] - want).max() > 0.1
    # rays that enter the kept part at the box face keep the gradient normal
    face = (out["iter"] == 0.0)
    assert np.array_equal(out["normal"][face], uncut["normal"][face]) and (out["cap"][face] == -1).all()


# ---- 3: what the kernels build their interval on ----------------------------------------------------------------------
def test_the_predicate_is_monotone_along_every_ray_in_f32():
    rng = np.random.default_rng(20240611)
    world = tilted_world()
    runs = 0
    for view in ("+x", "-z", "angled", "perspective"):
        if view == "angled":
            from test_iso import angled
            spec = spec_for(angled)
        elif view == "perspective":
            spec = spec_for("+z")
            spec.projection, spec.fov = "perspective", 40.0
        else:
            spec = spec_for(view)
        M = matrices(spec, world if view != "+x" else None)
        with np.errstate(all="ignore"):
            S = iso_twin.setup_rays(M, SIZE, material(), FRAME, FRAME, None)
        assert S["frag"].sum() > 100
        for _ in range(6):
            K = int(rng.integers(1, 9))
            normals = rng.normal(size=(K, 3))
            through = np.full(3, 15.5) + rng.normal(scale=6.0, size=(K, 3))
            planes = np.concatenate([normals, (normals * through).sum(1, keepdims=True)], axis=1)
            planes *= rng.choice([1e-3, 1.0, 1e3], size=(K, 1))
            rc = cut_twin.RayCut(S, planes, "ANY")
            n = S["nsteps"]
            i = np.arange(int(n.max()), dtype=f32)
            valid = S["frag"][..., None] & (i < n[..., None])
            behind = []
            for k in range(K):
                E = rc.A[k][..., None] + i * rc.B[k][..., None]
                assert E.dtype == f32
                dE = np.diff(E, axis=-1)
                ok = valid[..., 1:]
                rising, falling = ((dE >= 0) | ~ok).all(-1), ((dE <= 0) | ~ok).all(-1)
                assert (rising | falling)[S["frag"]].all()
                b = (E < 0) & valid
                behind.append(b)
                # a prefix or a suffix: at most one change along the ray
                assert (np.abs(np.diff(b.astype(np.int8), axis=-1)) * ok).sum(-1).max() <= 1
            kept = valid & ~np.logical_or.reduce(behind)
            cut_all = valid & np.logical_and.reduce(behind)
            for s in (kept, cut_all):                         # single intervals: at most one rise and one fall
                edges = np.diff(np.pad(s.astype(np.int8), [(0, 0)] * (s.ndim - 1) + [(1, 1)]), axis=-1)
                assert (edges == 1).sum(-1).max() <= 1
            runs += 1
    assert runs == 24


# ---- 4, 5, 6 ---------------------------------------------------------------------------------------------------------
def _scene():
    """A block with structure: a dense half behind a labelled wall, a finer LOD over part of it."""
    d = step_along_x(12)
    d[:, 10:20, 6:8] = 150
    labels = (np.arange(N)[:, None, None] // 8 + np.zeros((N, N, N))).astype(np.uint32)
    coarse = np.full((16, 16, 16), 120, np.uint8)
    rings = [ring(d, labels, z_range=(4, 24)), ring(coarse, np.full((16, 16, 16), 9, np.uint32), scale=0.5)]
    from test_iso import angled
    return rings, matrices(spec_for(angled), tilted_world())


TABLE = np.array([(0.1, 0.2, 0.9, 0.0), (0.9, 0.5, 0.1, 0.15), (1.0, 1.0, 0.4, 0.6)], f32)


def comp(rings, M, planes, mode="ANY", linear=False, tint=False):
    mat = material(clim=(0.0, 255.0))
    return composite_twin.composite_twin(rings, M, SIZE, mat, TABLE, FRAME, FRAME, 0.95, tint, pick_id=5,
                                         cut_planes=planes, cut_mode=mode, linear=linear)


@pytest.mark.parametrize("linear", [False, True])
def test_planes_that_cut_nothing_give_the_uncut_twins_bit_for_bit(linear):
    rings, M = _scene()
    far = [(1.0, 0.0, 0.0, -1000.0), (0.0, -1.0, 0.2, -1000.0)]
    mat = material(clim=(0.0, 255.0))
    for tint in (False, True):
        fn = linear_twin.composite_linear if linear else composite_twin.composite_twin
        want = fn(rings, M, SIZE, mat, TABLE, FRAME, FRAME, 0.95, tint, pick_id=5)
        assert (want["flags"] == HIT).sum() > 100
        for planes, mode in (([], "ANY"), ([], "ALL"), (far, "ANY"), (far, "ALL"), (far[:1] + [(1.0, 0.0, 0.0, 1000.0)], "ALL")):
            got = comp(rings, M, planes, mode, linear, tint)
            for k in want:
                assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (k, planes, mode)
    for params in (dict(iso_value=100.0, refine=4), dict(iso_value=130.0, refine=0, color_by_label=True)):
        fn = linear_twin.iso_linear if linear else iso_twin.iso_twin
        want = fn(rings, M, SIZE, material(), FRAME, FRAME, dict(SHADE, **params), pick_id=5)
        assert (want["flags"] == HIT).sum() > 100
        for planes, mode in (([], "ANY"), (far, "ANY"), (far, "ALL")):
            got = iso(rings, M, planes, mode, linear, **params)
            assert (got["cap"] == -1).all()
            for k in want:
                assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (k, planes, mode)


def test_planes_that_cut_everything_miss_on_every_fragment():
    rings, M = _scene()
    S = iso_twin.setup_rays(M, SIZE, material(), FRAME, FRAME, None)
    frag = S["frag"]
    assert frag.sum() > 100
    for planes, mode in (([(1.0, 0.0, 0.0, 1000.0)], "ANY"), ([(1.0, 0.0, 0.0, 1000.0), (0.0, 1.0, 0.0, 1000.0)], "ALL"),
                         ([(1.0, 0.0, 0.0, -1000.0), (0.0, 1.0, 0.0, 1000.0)], "ANY")):
        for out in (iso(rings, M, planes, mode, iso_value=100.0, refine=4), comp(rings, M, planes, mode)):
            assert np.array_equal(out["flags"], np.where(frag, MISS, DISCARD))
            assert np.array_equal(out["steps"], np.where(frag, S["nsteps"], 0))
            for k in ("rgba", "depth", "label", "pick"):
                assert not out[k].any(), k


@pytest.mark.parametrize("linear", [False, True])
def test_one_plane_under_any_equals_one_plane_under_all(linear):
    rings, M = _scene()
    plane = [(0.8, -0.36, -0.48, 0.8 * 15.5 - 0.36 * 15.5 - 0.48 * 15.5 + 1.0)]
    a, b = (iso(rings, M, plane, mode, linear, iso_value=100.0, refine=4) for mode in ("ANY", "ALL"))
    assert (a["cap"] == 0).sum() > 20 and (a["flags"] == HIT).sum() > 100
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    a, b = (comp(rings, M, plane, mode, linear, tint=True) for mode in ("ANY", "ALL"))
    assert (a["flags"] == HIT).sum() > 100
    uncut = comp(rings, M, [], "ANY", linear, tint=True)
    assert (a["rgba"] != uncut["rgba"]).any(-1).sum() > 50
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_a_composite_ray_cut_in_the_middle_composes_the_two_outer_runs_in_order():
    d = np.full((N, N, N), 10, np.uint8)
    d[:, :, 16:] = 200
    spec = spec_for("+x")
    # behind both planes: world x in (10.2, 20.3), i.e. the samples i with 10.7 < i * 32 / 113 < 20.8: 38 .. 73
    planes = [(-1.0, 0.0, 0.0, -10.2), (1.0, 0.0, 0.0, 20.3)]
    T = np.array([(0.2, 0.4, 0.9, 0.0), (1.0, 0.3, 0.1, 0.25)], f32)
    mat = material(clim=(0.0, 255.0))
    out = composite_twin.composite_twin([ring(d)], spec.matrices(), SIZE, mat, T, FRAME, FRAME, 0.999, cut_planes=planes, cut_mode="ALL")
    kept = [i for i in range(NSTEPS) if not 38 <= i <= 73]
    R = G = B = A = f32(0.0)
    w_best, best = f32(0.0), -1
    for i in kept:                                            # by hand, in f32, over the kept samples alone
        s = f32(10.0 if i * N / NSTEPS < 16.0 else 200.0)
        f = (s - f32(0.0)) / (f32(255.0) - f32(0.0)) * f32(1.0)
        e = [T[0, c] + f * (T[1, c] - T[0, c]) for c in range(4)]
        w = (f32(1.0) - A) * e[3]
        R, G, B, A = R + w * e[0], G + w * e[1], B + w * e[2], A + w
        if w > w_best:
            w_best, best = w, i
        last = i
        if A >= f32(0.999):
            break
    assert best == 74                                         # the first sample of the far run outweighs the near run's
    assert 74 < last < NSTEPS - 1                             # the ray ends at the cutoff, inside the far run
    assert (out["flags"] == HIT).all() and (out["steps"] == last + 1).all()     # the cut samples are counted
    assert (out["first"] == 0).all() and (out["best"] == best).all()
    want = np.array([R / A, G / A, B / A, A * f32(0.75)], f32)
    assert np.abs(out["rgba"] - want).max() <= 1e-6
    word = int(out["pick"][0, 0])
    assert (word >> 20) & 0x3FFF == int(f32(best) * f32(1.0 / NSTEPS) * f32(16383.0)) or \
        abs(((word >> 20) & 0x3FFF) - best / NSTEPS * 16383.0) <= 1.0
    uncut = composite_twin.composite_twin([ring(d)], spec.matrices(), SIZE, mat, T, FRAME, FRAME, 0.999)
    assert np.abs(uncut["rgba"] - out["rgba"]).max() > 1e-2
    # under ANY the same two planes keep nothing (no point is in front of both), and a cut-off first half moves `first`
    half = composite_twin.composite_twin([ring(d)], spec.matrices(), SIZE, mat, T, FRAME, FRAME, 0.999, cut_planes=planes[1:])
    assert (half["first"] == 74).all() and (half["steps"] > 74).all()


# ---- 8, 9: the Python surface -----------------------------------------------------------------------------------------
def test_material_cut_planes_and_mode():
    m = SubVolumeMaterial(0.5)
    assert m.cut_planes == [] and m.cut_mode == "ANY" and SubVolumeMaterial.MAX_CUT_PLANES == 8
    v = m._version
    m.cut_planes = [(1, 0, 0, 2.5), [0.0, -2.0, 0.0, 1.0]]
    assert m.cut_planes == [(1.0, 0.0, 0.0, 2.5), (0.0, -2.0, 0.0, 1.0)] and m._version > v
    m.cut_mode = "all"
    assert m.cut_mode == "ALL"
    m.cut_planes = [(0.0, 0.0, 1.0, float(k)) for k in range(8)]
    kept, v = m.cut_planes, m._version
    for bad in ([(1.0, 0.0, 0.0)], ["abcd"], [(1.0, 0.0, 0.0, 0.0, 0.0)]):
        with pytest.raises(TypeError, match="abcd tuple"):
            m.cut_planes = bad
    for bad in ([(0.0, 0.0, 1.0, 0.0)] * 9, [(float("nan"), 0.0, 1.0, 0.0)], [(1.0, 0.0, 0.0, float("inf"))],
                [(0.0, 0.0, 0.0, 1.0)], [(1e30, 1e30, 0.0, 0.0)], [(1e-30, 0.0, 0.0, 0.0)], [(1e39, 0.0, 0.0, 0.0)]):
        with pytest.raises(ValueError):
            m.cut_planes = bad
    with pytest.raises(ValueError, match="cut_mode"):
        m.cut_mode = "SOME"
    assert m.cut_planes == kept and m._version == v and m.cut_mode == "ALL"
    m.cut_planes = ()
    assert m.cut_planes == []
    # the clipping planes are a separate property
    assert m.clipping_planes == [] and m.clipping_mode == "ANY"


def small_volume():
    d = np.zeros((16, 16, 16), np.uint8)
    return SubVolume(SubVolumeMaterial(0.5), [(d, d)], (2, 2, 2), (4, 4, 4))


@pytest.mark.parametrize("mode", ["lmip", "mip", "weighted_average"])
def test_the_march_refuses_cut_planes_before_any_device_work(mode, monkeypatch):
    vol = small_volume()
    touched = []
    monkeypatch.setattr(vol, "prepare", lambda: touched.append(1))
    vol.material.render_mode = mode
    vol.material.cut_planes = [(1.0, 0.0, 0.0, 4.0)]
    with pytest.raises(ValueError) as e:
        vol.render(object(), 8, 6)
    msg = str(e.value)
    assert "cut planes" in msg and "composite" in msg and "iso" in msg and "svr_composite" in msg
    assert not touched


def test_crop_planes_classify_points_under_a_tilted_world():
    vol = small_volume()
    w = tilted_world()
    vol.world.rotation_matrix = w.rotation_matrix
    vol.world.scale, vol.world.position = w.scale, w.position
    begin, end = (2, 5, 3), (9, 11, 14)                      # numpy order
    planes = np.array(vol.crop_planes(begin, end))
    assert planes.shape == (6, 4) and planes.dtype == np.float64
    rng = np.random.default_rng(7)
    idx = rng.uniform(-3.0, 19.0, size=(4000, 3))            # continuous voxel coordinates, numpy order
    margin = np.minimum(np.abs(idx - (np.array(begin) - 0.5)), np.abs(idx - (np.array(end) - 0.5))).min(1)
    idx = idx[margin > 1e-6]
    inside = ((idx >= np.array(begin) - 0.5) & (idx < np.array(end) - 0.5)).all(1)
    assert 100 < inside.sum() < len(idx) - 100
    world_pts = (np.asarray(vol.world.matrix) @ np.c_[idx[:, ::-1], np.ones(len(idx))].T).T[:, :3]
    behind_any = ((world_pts @ planes[:, :3].T) < planes[:, 3]).any(1)
    assert np.array_equal(~behind_any, inside)
    # voxel centres of the box are kept, their neighbours outside are not
    for bad in (((1, 2), (3, 4, 5)), ((0, 0, 0), (4, 0, 4)), ((0, 0, float("nan")), (1, 1, 1))):
        with pytest.raises(ValueError):
            vol.crop_planes(*bad)
    vol.material.cut_planes, vol.material.cut_mode = vol.crop_planes(begin, end), "ANY"       # the material takes them
    assert len(vol.material.cut_planes) == 6


# ---- 10 ---------------------------------------------------------------------------------------------------------------
def test_svr_set_cut_planes_is_declared_bound_and_exported():
    raw = open(os.path.join(ROOT, "include", "svr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+svr_set_cut_planes\s*\(\s*svr_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*planes\s*,\s*"
                     r"uint32_t\s+count\s*,\s*int\s+mode\s*\)", text)
    assert re.search(r"#define\s+SVR_MAX_CUT_PLANES\s+8\b", text)
    assert re.search(r"#define\s+SVR_CUT_ANY\s+0\b", text) and re.search(r"#define\s+SVR_CUT_ALL\s+1\b", text)
    assert int(re.search(r"#define SVR_ABI_VERSION (\d+)", text).group(1)) == 9
    assert _native.SIGNATURES["svr_set_cut_planes"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                                                       ctypes.c_uint32, ctypes.c_int])
    assert _native.CUT_MODES == {"ANY": 0, "ALL": 1} and _native.MAX_CUT_PLANES == 8
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "svr_set_cut_planes")
    # no existing struct gained a field
    assert ctypes.sizeof(_native.IsoParams) == 80 and ctypes.sizeof(_native.CompositeParams) == 8
