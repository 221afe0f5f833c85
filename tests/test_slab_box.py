"""The packed bounding box of a brick slab (csrc/slab_box.h): a lane packs the ends of its samples into three words of
two signed 16-bit halves, the wave reduces them with packed minima, and the scalar side unpacks six bounds.  The header
is plain C++; it is compiled here on its own with the host compiler.  The driver restates the wave's reduction over 64
array slots in the order the kernel runs it (half swap, row swap, four steps inside a row) and prints the box; the
tests hold it to six independent min / max reductions done here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")

# box: reads cases from stdin, one per line: 64 x "<live> <x0> <x1> <y0> <y1> <z0> <z1>" (the ends as integers; the driver
#      hands them on as floats with a fraction, as the march does), prints "<none> lx ly lz hx hy hz" per case
# pred <off> <shape>: "<0|1>";  mode <o0> <o1> <o2> <s0> <s1> <s2>: "packed" | "unpacked"
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "slab_box.h"
// v_permlane32_swap_b32 d, s: lanes 32-63 of d change places with lanes 0-31 of s
static void swap32(uint32_t* d, uint32_t* s) { for (int i = 0; i < 32; ++i) { const uint32_t t = d[32 + i]; d[32 + i] = s[i]; s[i] = t; } }
// v_permlane16_swap_b32 d, s: rows 1 and 3 of d change places with rows 0 and 2 of s
static void swap16(uint32_t* d, uint32_t* s) {
    for (int r = 0; r < 4; r += 2) for (int i = 0; i < 16; ++i) { const uint32_t t = d[16 * (r + 1) + i]; d[16 * (r + 1) + i] = s[16 * r + i]; s[16 * r + i] = t; }
}
static void step(uint32_t* r, int (*from)(int)) {
    uint32_t m[64];
    for (int i = 0; i < 64; ++i) m[i] = r[from(i)];
    for (int i = 0; i < 64; ++i) r[i] = svr_slab_box_min2(r[i], m[i]);
}
static int xor1(int i) { return i ^ 1; }
static int xor2(int i) { return i ^ 2; }
static int half_mirror(int i) { return (i & ~7) | (7 - (i & 7)); }
static int mirror(int i) { return (i & ~15) | (15 - (i & 15)); }
static svr_slab_box reduce(const svr_slab_box_words* w) {
    uint32_t a[64], b[64], c[64], r[64];
    for (int i = 0; i < 64; ++i) { a[i] = w[i].a; b[i] = w[i].b; c[i] = w[i].c; }
    swap32(a, b);
    for (int i = 0; i < 64; ++i) a[i] = svr_slab_box_min2(a[i], b[i]);
    swap16(a, c);
    for (int i = 0; i < 64; ++i) r[i] = svr_slab_box_min2(a[i], c[i]);
    step(r, xor1); step(r, xor2); step(r, half_mirror); step(r, mirror);
    for (int i = 0; i < 64; ++i) if (r[i] != r[i & ~15]) { fprintf(stderr, "row not uniform\n"); exit(4); }
    return svr_slab_box_unpack(r[0], r[32], r[16], r[48]);
}
int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "pred")) { printf("%d\n", svr_slab_box_fits16(atoll(argv[2]), atoll(argv[3])) ? 1 : 0); return 0; }
    if (argc == 8 && !strcmp(argv[1], "mode")) {
        const int32_t off[3] = { atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) };
        const uint32_t shape[3] = { (uint32_t)atoll(argv[5]), (uint32_t)atoll(argv[6]), (uint32_t)atoll(argv[7]) };
        printf("%s\n", svr_slab_box_mode_of(off, shape) == SVR_SLAB_BOX_PACKED ? "packed" : "unpacked");
        return 0;
    }
    if (argc != 2 || strcmp(argv[1], "box")) return 3;
    for (;;) {
        svr_slab_box_words w[64];
        for (int i = 0; i < 64; ++i) {
            int live, e[6];
            if (scanf("%d %d %d %d %d %d %d", &live, &e[0], &e[1], &e[2], &e[3], &e[4], &e[5]) != 7) return i == 0 ? 0 : 5;
            // a fraction on every end: the pack truncates, as the march's converts do
            w[i] = svr_slab_box_pack(e[0] + 0.25f, e[1] + 0.75f, e[2] + 0.5f, e[3] + 0.0f, e[4] + 0.125f, e[5] + 0.875f, live != 0);
        }
        const svr_slab_box b = reduce(w);
        printf("%d %d %d %d %d %d %d\n", b.none ? 1 : 0, b.lx, b.ly, b.lz, b.hx, b.hy, b.hz);
    }
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("slab_box")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def boxes(driver, cases):
    """cases: list of (live[64] bool, ends[64, 6] int) -> list of (none, lx, ly, lz, hx, hy, hz)"""
    text = "".join("%d %d %d %d %d %d %d\n" % (int(lv), *row) for live, ends in cases for lv, row in zip(live, ends.tolist()))
    out = subprocess.run([driver, "box"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return [tuple(int(v) for v in line.split()) for line in out if line]


def expected(live, ends):
    """six independent reductions over the live lanes: min of both ends per axis, max of both ends per axis"""
    if not live.any():
        return None
    e = ends[live]
    lo = np.minimum(e[:, 0::2], e[:, 1::2]).min(axis=0)
    hi = np.maximum(e[:, 0::2], e[:, 1::2]).max(axis=0)
    return (0, int(lo[0]), int(lo[1]), int(lo[2]), int(hi[0]), int(hi[1]), int(hi[2]))


def check(driver, cases):
    got = boxes(driver, cases)
    assert len(got) == len(cases)
    for (live, ends), g in zip(cases, got):
        want = expected(live, ends)
        if want is None:
            assert g[0] == 1, g
        else:
            assert g == want, (g, want, np.flatnonzero(live))


def test_random_boxes_and_live_masks(driver):
    rng = np.random.default_rng(7)
    cases = []
    for k in range(300):
        span = int(rng.choice([1, 2, 17, 300, 32768]))
        base = int(rng.integers(0, 32768 - span + 1))
        ends = rng.integers(base, base + span, size=(64, 6))
        density = rng.choice([0.02, 0.5, 0.98, 1.0])
        live = rng.random(64) < density
        cases.append((live, ends))
    check(driver, cases)


def test_one_live_lane_at_every_position_and_none(driver):
    rng = np.random.default_rng(11)
    cases = []
    for lane in range(64):
        live = np.zeros(64, bool)
        live[lane] = True
        cases.append((live, rng.integers(0, 32768, size=(64, 6))))      # the dead lanes hold values that must not show
    cases.append((np.zeros(64, bool), rng.integers(0, 32768, size=(64, 6))))
    cases.append((np.zeros(64, bool), np.zeros((64, 6), np.int64)))
    check(driver, cases)


def test_values_on_the_edges_of_the_range(driver):
    rng = np.random.default_rng(13)
    edge = np.array([0, 1, 32766, 32767])
    cases = []
    for k in range(200):
        ends = edge[rng.integers(0, 4, size=(64, 6))]
        live = rng.random(64) < rng.choice([0.05, 0.6, 1.0])
        cases.append((live, ends))
    for v in edge:                                                       # a wave that sits on one edge value altogether
        cases.append((np.ones(64, bool), np.full((64, 6), v)))
        one = np.zeros(64, bool)
        one[int(rng.integers(0, 64))] = True
        cases.append((one, np.full((64, 6), v)))
    # the low bound on the top edge and the high bound on the bottom edge, per axis, against the sentinel
    cases.append((np.ones(64, bool), np.tile(np.array([32767, 32767, 0, 0, 32767, 0]), (64, 1))))
    check(driver, cases)


def test_all_lanes_equal(driver):
    rng = np.random.default_rng(17)
    cases = []
    for k in range(50):
        row = rng.integers(0, 32768, size=6)
        cases.append((np.ones(64, bool), np.tile(row, (64, 1))))
        cases.append((rng.random(64) < 0.5, np.tile(row, (64, 1))))
    check(driver, cases)


def test_predicate_at_the_16_bit_edge(driver):
    def pred(off, shape):
        return subprocess.run([driver, "pred", str(off), str(shape)], capture_output=True, text=True, check=True).stdout.strip() == "1"
    assert pred(0, 32767)
    assert not pred(0, 32768)
    assert pred(32000, 767) and not pred(32000, 768)
    assert not pred(-1, 10)                       # indices are taken as non-negative
    assert not pred(0, 1 << 31)


def test_a_ring_that_fails_the_predicate_reports_unpacked(driver):
    def mode(off, shape):
        return subprocess.run([driver, "mode", *map(str, off), *map(str, shape)], capture_output=True, text=True, check=True).stdout.strip()
    assert mode((0, 0, 0), (32767, 1024, 1024)) == "packed"
    assert mode((0, 0, 0), (1024, 32768, 1024)) == "unpacked"
    assert mode((0, 0, 40000), (1024, 1024, 1024)) == "unpacked"
    assert mode((100, 200, 300), (1024, 1024, 1024)) == "packed"
