"""CPU: how a density ring of 4 GiB or more is cut into buffer resources (csrc/ring_parts.h, the one function that
decides it for `span_addressable` and `fill_params`).  The header is compiled here with g++ and called through ctypes:
invariants over a sweep of storages, copies, plane sizes at every split from 1 to 9 planes, and ring z extents of 7, 8
and 9 parts; hand-derived known answers; SVR_FORCE_ZSPLIT with a copy."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sub_volume_renderer_amd", "csrc")
LIMIT = (1 << 32) - 128              # a part's bytes + its 64 bytes of slack stay below 2^32
BLOCK_Z = {1: 4, 2: 4, 4: 2}         # ring z planes per micro-block of the copy (include/svr.h, blocked_twin)
FIELDS = ("nparts", "zsplit", "part_bytes", "rbytes", "rbytes_last", "span_ok", "twin_ok")

DRIVER = r"""
#include "ring_parts.h"
extern "C" void ring_parts_c(uint32_t rx, uint32_t ry, uint32_t rz, uint32_t esize, int twin, int force_zsplit,
                             uint32_t out[7]) {
    const RingParts r = ring_parts(rx, ry, rz, esize, twin != 0, force_zsplit);
    out[0] = r.nparts; out[1] = r.zsplit; out[2] = r.part_bytes; out[3] = r.rbytes; out[4] = r.rbytes_last;
    out[5] = r.span_ok ? 1u : 0u; out[6] = r.twin_ok ? 1u : 0u;
}
"""


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to compile csrc/ring_parts.h on its own")
    d = tmp_path_factory.mktemp("ring_parts")
    src, lib = d / "driver.cpp", d / "libring_parts.so"
    src.write_text(DRIVER)
    # plain host C++: no HIP header, no HIP compiler
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I", CSRC,
                    str(src), "-o", str(lib)], check=True)
    so = ctypes.CDLL(str(lib))
    so.ring_parts_c.restype = None
    so.ring_parts_c.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]

    def call(ring_xyz, esize, twin=False, force_zsplit=0):
        out = (ctypes.c_uint32 * 7)()
        so.ring_parts_c(*ring_xyz, esize, int(twin), force_zsplit, out)
        r = dict(zip(FIELDS, out))
        r["span_ok"], r["twin_ok"] = bool(r["span_ok"]), bool(r["twin_ok"])
        return r

    return call


def _holds_whole_blocks(ring_xyz, esize, r):
    """Independently of the function: does every part of the micro-block copy (the ring's parts laid over the copy:
    part p from p * part_bytes, as the march indexes it) hold every block of the planes of that part whole?"""
    rx, ry, rz = ring_xyz
    plane, bz = rx * ry * esize, BLOCK_Z[esize]
    if r["nparts"] == 1:
        return True
    for p in range(r["nparts"]):
        lo = p * r["zsplit"]
        hi = min(rz, lo + r["zsplit"])                      # planes [lo, hi) of part p
        start = p * r["part_bytes"]
        size = r["rbytes_last"] - 64 if p == r["nparts"] - 1 else r["rbytes"]     # (a full part's resource: no slack)
        # the copy's bytes of planes lo .. hi - 1: whole blocks of bz planes, from block lo // bz to (hi - 1) // bz
        first, last = (lo // bz) * bz * plane, ((hi - 1) // bz + 1) * bz * plane
        if first < start or last > start + size:
            return False
    return True


def _check_invariants(ring_xyz, esize, twin, r):
    rx, ry, rz = ring_xyz
    plane, nbytes = rx * ry * esize, rx * ry * rz * esize
    what = (ring_xyz, esize, twin, r)
    if plane > LIMIT:                                       # not one plane fits a resource: only 64-bit addressing
        assert not r["span_ok"] and not r["twin_ok"], what
        return
    n, z = r["nparts"], r["zsplit"]
    # the parts tile [0, ring_z) in whole planes
    assert 1 <= n and 1 <= z <= rz, what
    assert (n - 1) * z < rz <= n * z, what
    if nbytes + 64 < (1 << 32):
        assert n == 1 and z == rz and r["part_bytes"] == 0 and r["rbytes"] == r["rbytes_last"] == nbytes + 64, what
    else:
        assert n >= 2, what
    if n > 1:
        assert r["part_bytes"] == r["rbytes"] == z * plane, what
        assert z < 4 or z % 4 == 0, what                    # parts of 4 planes or more: a multiple of 4
    # every resource below 2^32 (the u32 fields hold the exact sizes, nothing wrapped)
    assert z * plane + 64 < (1 << 32) or n == 1, what
    assert r["rbytes"] < (1 << 32) and r["rbytes_last"] < (1 << 32), what
    # the last resource covers the last part and its 64 bytes of slack, exactly
    assert r["rbytes_last"] == nbytes - (n - 1) * z * plane + 64, what
    assert r["rbytes_last"] >= (rz - (n - 1) * z) * plane + 64, what
    # the span kernel: at most 8 parts and the 24-bit row index / row pitch — and nothing else holds it back
    fits24 = ry * rz < (1 << 24) and rx * esize < (1 << 24)
    assert r["span_ok"] == (n <= 8 and fits24), what
    # the copy: used only where every part holds whole blocks of it, and used wherever they do
    assert r["twin_ok"] == (twin and _holds_whole_blocks(ring_xyz, esize, r)), what
    if r["twin_ok"] and n > 1:
        assert z % BLOCK_Z[esize] == 0, what


def _sweep():
    """(ring_xyz, esize) over planes just below and just above (2^32 - 128) / k for k = 1 .. 9 (the plane sizes at which
    zsplit changes) and ring z extents that give 7, 8 and 9 parts; ring extents keep the copy's (8, 4, 4) grain."""
    cases = []
    for esize in (1, 2, 4):
        rx = 16384
        for k in range(1, 10):
            t = LIMIT // k
            below = (t // (esize * rx)) // 4 * 4            # ry: the largest multiple of 4 with a plane <= t
            for ry in (below, below + 4):
                plane = rx * ry * esize
                assert (plane <= t) == (ry == below)
                zs = min(LIMIT // plane, 1 << 20)
                zs = zs & ~3 if zs >= 4 else zs
                for parts in (1, 2, 7, 8, 9):
                    rz = max(1, (parts - 1) * zs + 1)
                    cases.append(((rx, ry, rz), esize))
                    cases.append(((rx, ry, -(-rz // 4) * 4), esize))     # the copy's grain
    # rings just below and just above 4 GiB (one resource / two parts), and at the edge of the 64 bytes of slack
    for esize in (1, 2, 4):
        for rz in (252, 255, 256, 257, 260):
            cases.append(((4096 // esize, 4096, rz), esize))
    cases += [((16, 1, (1 << 26) - 2), 4), ((16, 1, (1 << 26) - 1), 4), ((16, 1, 1 << 26), 4)]
    cases += [((65536, 65536, 4), 1), ((65536, 32768, 2), 4), ((32768, 32768, 8), 4)]         # planes of 4 GiB and more
    return cases


def test_invariants_over_plane_sizes_at_every_split_and_7_8_9_parts(parts):
    seen = set()
    for ring_xyz, esize in _sweep():
        # (a copy needs ring extents that are multiples of (8, 4, 4): svr_create refuses it otherwise)
        grain = ring_xyz[0] % 8 == 0 and ring_xyz[1] % 4 == 0 and ring_xyz[2] % 4 == 0
        for twin in (False, True) if grain else (False,):
            r = parts(ring_xyz, esize, twin)
            _check_invariants(ring_xyz, esize, twin, r)
            seen.add((r["zsplit"] if r["nparts"] > 1 else 0, min(r["nparts"], 10)))
    assert {z for z, _ in seen} >= {1, 2, 3, 4, 8}, seen                # every kind of split came up
    assert {n for _, n in seen} >= {1, 2, 7, 8, 9}, seen


# (x, y, z), bytes per voxel, copy -> zsplit, parts, span kernel, march uses the copy (None: no copy asked for)
KNOWN = [
    ((2112, 1024, 1024), 4, True, 496, 3, True, True),       # test_gpu_streaming's 8.86 GB float ring
    ((65536, 4096, 4), 4, True, 3, 2, True, False),          # 1 GiB float planes: parts of 3 cut the copy's 2-plane blocks
    ((65536, 6144, 4), 4, True, 2, 2, True, True),           # 1.5 GiB float planes: parts of 2 = whole blocks
    ((65536, 12288, 4), 2, True, 2, 2, True, False),         # 1.5 GiB uint16 planes: parts of 2 cut 4-plane blocks
    ((65536, 32768, 4), 1, True, 1, 4, True, False),         # 2 GiB byte planes: parts of 1
    ((65536, 8192, 32), 1, False, 4, 8, True, None),         # the span kernel's most parts
    ((65536, 8192, 33), 1, False, 4, 9, False, None),        # one more: march_simple
    ((4096, 4096, 256), 1, True, 252, 2, True, True),        # exactly 4 GiB
    # the scenes of tests/test_gpu_big_ring_parts.py (extents below 2^15, where the span kernel runs direct batches)
    ((16384, 16384, 4), 4, True, 3, 2, True, False),
    ((28672, 28672, 4), 2, True, 2, 2, True, False),
    ((20480, 20480, 4), 4, True, 2, 2, True, True),
    ((23168, 23176, 32), 1, False, 4, 8, True, None),
    ((23168, 23176, 33), 1, False, 4, 9, False, None),
]


@pytest.mark.parametrize("ring_xyz,esize,twin,zsplit,nparts,span_ok,twin_ok", KNOWN, ids=[
    f"{'x'.join(map(str, k[0]))}-{k[1]}B" for k in KNOWN])
def test_known_answers(parts, ring_xyz, esize, twin, zsplit, nparts, span_ok, twin_ok):
    r = parts(ring_xyz, esize, twin)
    assert (r["zsplit"], r["nparts"], r["span_ok"]) == (zsplit, nparts, span_ok), r
    assert r["twin_ok"] == bool(twin_ok), r
    _check_invariants(ring_xyz, esize, twin, r)
    if twin_ok is None:
        assert not parts(ring_xyz, esize, False)["twin_ok"]


def test_a_ring_below_4_gib_is_one_resource_and_keeps_its_copy(parts):
    for esize in (1, 2, 4):
        r = parts((1024 // esize * 8, 1024, 64), esize, True)
        assert (r["nparts"], r["zsplit"], r["part_bytes"]) == (1, 64, 0) and r["span_ok"] and r["twin_ok"], r
        assert r["rbytes"] == r["rbytes_last"] == 1024 * 8 * 1024 * 64 + 64


@pytest.mark.parametrize("esize", [1, 2, 4])
def test_forced_splits_with_a_copy_keep_whole_blocks(parts, esize):
    """SVR_FORCE_ZSPLIT (-DSVR_EXPERIMENTS builds) cuts rings of any size: with a copy every forced part size still
    gives whole blocks, at most 8 parts, and the invariants of the production split."""
    for ring_xyz in ((64, 32, 32), (40, 12, 44), (24, 8, 4)):
        for force in range(1, ring_xyz[2] + 2):
            r = parts(ring_xyz, esize, True, force)
            what = (ring_xyz, esize, force, r)
            assert r["twin_ok"] and r["nparts"] <= 8 and r["span_ok"], what
            assert r["nparts"] == 1 or r["zsplit"] % 4 == 0, what
            assert (r["nparts"] - 1) * r["zsplit"] < ring_xyz[2] <= r["nparts"] * r["zsplit"], what
            assert _holds_whole_blocks(ring_xyz, esize, r), what
            assert r["rbytes_last"] == ring_xyz[0] * ring_xyz[1] * esize * (ring_xyz[2] - (r["nparts"] - 1) * r["zsplit"]) + 64
            # without a copy the part size is the forced one (at least an eighth of the ring), not rounded
            q = parts(ring_xyz, esize, False, force)
            assert q["zsplit"] == min(ring_xyz[2], max(force, -(-ring_xyz[2] // 8))), (what, q)


def test_the_host_derives_the_split_in_one_place():
    """span_addressable() and fill_params() take the split from ring_parts(); nothing else in the host code computes it,
    and edits to the header rebuild the library."""
    import inspect

    import __graft_entry__ as g

    units = {name: open(os.path.join(CSRC, name)).read() for name in g.HIP_SOURCES if name.startswith("svr_")}
    assert set(units) == {"svr_api.hip", "svr_upload.hip", "svr_render.hip", "svr_modes.hip"}     # the host units
    render = units["svr_render.hip"]
    assert '#include "ring_parts.h"' in render and "ring_parts(" in render
    for name, text in units.items():
        assert "- 128) / plane" not in text and "zsplit &=" not in text, name
        assert name == "svr_render.hip" or "ring_parts" not in text, name
    assert "ring_parts.h" in inspect.getsource(g.build_hip)
