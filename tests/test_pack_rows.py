"""The host half of an upload (csrc/pack_rows.h): rows of a strided host block gathered into a packed buffer by a few kept
threads.  The header is plain host C++; it is compiled here on its own with the host compiler.  The driver reads the
source blocks from files, packs the row ranges listed on stdin and writes the packed bytes to stdout; the tests hold them
to numpy's gather of the same strided view.  SVR_PACK_THREADS travels in the driver's environment.  Strides may be
negative (element (0, 0, 0) then lies inside the file, at the byte offset the driver is given) or zero."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-pthread"]

# argv: density_file labels_file des les  shape[3] (x y z)  density strides[3]  label strides[3] (bytes per x, y, z step)  fork
#       byte offset of element (0, 0, 0) in the density file, in the labels file
# stdin, per case: use_density use_labels r0 r1 -> stdout: the packed density rows, then the packed label rows
# fork = 1: the first case is packed here, every later one in a child forked after it (which has to start threads of its own)
DRIVER = r"""
#include <inttypes.h>
#include <stdio.h>
#include <sys/wait.h>
#include <fstream>
#include <iterator>
#include "pack_rows.h"
static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
int main(int argc, char** argv) {
    if (argc != 17) return 2;
    const std::vector<char> dsrc = slurp(argv[1]), lsrc = slurp(argv[2]);
    const size_t des = (size_t)atoll(argv[3]), les = (size_t)atoll(argv[4]);
    int32_t shape[3]; int64_t dst[3], lst[3];
    for (int a = 0; a < 3; ++a) { shape[a] = atoi(argv[5 + a]); dst[a] = atoll(argv[8 + a]); lst[a] = atoll(argv[11 + a]); }
    const bool fork_after_first = atoi(argv[14]) != 0;
    const char* d0 = dsrc.data() + atoll(argv[15]);
    const char* l0 = lsrc.data() + atoll(argv[16]);
    int use_d, use_l, done = 0;
    int64_t r0, r1;
    while (scanf("%d %d %" SCNd64 " %" SCNd64, &use_d, &use_l, &r0, &r1) == 4) {
        if (fork_after_first && done == 1) {
            fflush(stdout);
            const pid_t child = fork();
            if (child < 0) return 3;
            if (child > 0) { int st = 0; waitpid(child, &st, 0); return WIFEXITED(st) ? WEXITSTATUS(st) : 4; }
        }
        const size_t n = (size_t)shape[0] * (size_t)(r1 - r0);
        std::vector<char> dout(use_d ? n * des : 0, (char)0x5A), lout(use_l ? n * les : 0, (char)0x5A);
        pack_rows(use_d ? d0 : nullptr, des, dst, dout.data(), use_l ? l0 : nullptr, les, lst, lout.data(), shape, r0, r1);
        if (use_d) fwrite(dout.data(), 1, dout.size(), stdout);
        if (use_l) fwrite(lout.data(), 1, lout.size(), stdout);
        ++done;
    }
    fflush(stdout);
    return 0;
}
"""

SHAPES = [(1, 1, 1), (3, 2, 5), (48, 7, 9), (528, 33, 40)]            # x, y, z
THREADS = ["1", "3", "16"]


def build_driver(directory, extra_flags=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = os.path.join(directory, "drv.cpp"), os.path.join(directory, "drv")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([cxx, *CXXFLAGS, *extra_flags, "-I", HEADER_DIR, src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("pack_rows")))


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    """Per shape and source kind: the files the driver reads and the strided views numpy gathers from.  The density is
    uint8 and the labels uint32 with different values, so that a mixed-up pointer or element size shows; the
    x-strided kind takes every other element of rows that are also padded at their end."""
    d = tmp_path_factory.mktemp("pack_rows_src")
    rng = np.random.default_rng(7)
    out = {}
    for shape in SHAPES:
        x, y, z = shape
        for kind in ("contiguous", "x-strided"):
            full = (z, y, x) if kind == "contiguous" else (z, y + 1, 2 * x + 3)
            views = []
            for name, dtype in (("density", np.uint8), ("labels", np.uint32)):
                base = rng.integers(0, np.iinfo(dtype).max, size=full, dtype=dtype, endpoint=True)
                path = str(d / ("%s_%s_%dx%dx%d.bin" % (name, kind, x, y, z)))
                base.tofile(path)
                view = base if kind == "contiguous" else base[:, :y, 0:2 * x:2]
                assert view.shape == (z, y, x)
                views.append((path, view))
            out[shape, kind] = views
    return out


def row_ranges(shape):
    """Whole blocks, ranges that start mid-plane (and end mid-plane), a single row; a row index is z * ny + y."""
    rows = shape[1] * shape[2]
    cand = [(0, rows), (shape[1] + 1, rows), (shape[1] // 2, rows - 1), (rows // 2, rows // 2 + 1), (rows - 1, rows)]
    return sorted({(a, b) for a, b in cand if 0 <= a < b <= rows})


def pack(driver, views, shape, cases, threads, fork=False, offsets=(0, 0)):
    """-> per case the packed (density, labels) bytes the driver wrote (None where that block was absent).
    offsets: where element (0, 0, 0) of each view lies in its file."""
    (dpath, dview), (lpath, lview) = views
    args = [driver, dpath, lpath, str(dview.itemsize), str(lview.itemsize), *map(str, shape), *(str(s) for s in dview.strides[::-1]),
            *(str(s) for s in lview.strides[::-1]), "1" if fork else "0", *map(str, offsets)]
    env = {k: v for k, v in os.environ.items() if k != "SVR_PACK_THREADS"}
    if threads is not None:
        env["SVR_PACK_THREADS"] = threads
    text = "".join("%d %d %d %d\n" % c for c in cases)
    raw = subprocess.run(args, input=text.encode(), capture_output=True, check=True, env=env).stdout
    got, at = [], 0
    for use_d, use_l, r0, r1 in cases:
        parts = []
        for use, view in ((use_d, dview), (use_l, lview)):
            n = shape[0] * (r1 - r0) * view.itemsize if use else 0
            parts.append(raw[at:at + n] if use else None)
            at += n
        got.append(tuple(parts))
    assert at == len(raw)
    return got


def expected(view, shape, r0, r1):
    """numpy's gather of the strided source: rows r0 .. r1 of the block, x fastest."""
    return np.ascontiguousarray(view).reshape(shape[1] * shape[2], shape[0])[r0:r1].tobytes()


def check(views, shape, cases, got):
    for (use_d, use_l, r0, r1), (dgot, lgot) in zip(cases, got):
        assert (dgot is not None) == bool(use_d) and (lgot is not None) == bool(use_l)
        if use_d:
            assert dgot == expected(views[0][1], shape, r0, r1), (shape, use_d, use_l, r0, r1)
        if use_l:
            assert lgot == expected(views[1][1], shape, r0, r1), (shape, use_d, use_l, r0, r1)


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("kind", ["contiguous", "x-strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_packed_rows_equal_numpys_gather(driver, sources, shape, kind, threads):
    views = sources[shape, kind]
    cases = [(use_d, use_l, r0, r1) for use_d, use_l in ((1, 0), (0, 1), (1, 1)) for r0, r1 in row_ranges(shape)]
    # (16 threads: more than rows / 2 for the two smallest blocks, which then pack with fewer)
    assert int(THREADS[-1]) > 2 * 5 // 2 and int(THREADS[-1]) < 7 * 9 // 2
    check(views, shape, cases, pack(driver, views, shape, cases, threads))


def test_default_thread_count(driver, sources):
    """Without SVR_PACK_THREADS: one thread per 512 KiB, at most 8 (3.3 MiB here; 15 KiB for the small block)."""
    for shape in ((528, 33, 40), (48, 7, 9)):
        views = sources[shape, "x-strided"]
        cases = [(1, 1, r0, r1) for r0, r1 in row_ranges(shape)]
        check(views, shape, cases, pack(driver, views, shape, cases, None))


@pytest.mark.parametrize("threads", ["3", "16"])
def test_a_forked_child_packs_with_threads_of_its_own(driver, sources, threads):
    shape = (528, 33, 40)
    views = sources[shape, "x-strided"]
    cases = [(1, 1, 0, 33 * 40), (1, 1, 34, 33 * 40), (0, 1, 0, 33 * 40), (1, 0, 700, 701)]
    check(views, shape, cases, pack(driver, views, shape, cases, threads, fork=True))


def address(a):
    return a.__array_interface__["data"][0]


@pytest.mark.parametrize("threads", ["1", "3"])
@pytest.mark.parametrize("kind", ["flip_x", "flip_y", "flip_z", "flip_all", "one_row", "one_plane"])
def test_negative_and_zero_strides(driver, tmp_path, kind, threads):
    """Sources flipped along each axis (negative strides: element (0, 0, 0) is the last of its axis in memory), one row
    broadcast over y (y stride 0) and one plane broadcast over z (z stride 0): the packed bytes == numpy's gather."""
    shape = (48, 7, 9)                                                   # x, y, z
    x, y, z = shape
    rng = np.random.default_rng(11)
    views, offsets = [], []
    for name, dtype in (("density", np.uint8), ("labels", np.uint32)):
        base = rng.integers(0, np.iinfo(dtype).max, size=(z, y, x), dtype=dtype, endpoint=True)
        view = {"flip_x": base[:, :, ::-1], "flip_y": base[:, ::-1], "flip_z": base[::-1], "flip_all": base[::-1, ::-1, ::-1],
                "one_row": np.broadcast_to(base[:, 3:4], base.shape), "one_plane": np.broadcast_to(base[5:6], base.shape)}[kind]
        path = str(tmp_path / (name + ".bin"))
        base.tofile(path)
        views.append((path, view))
        offsets.append(address(view) - address(base))
    sx, sy, sz = views[1][1].strides[::-1]
    assert {"flip_x": sx == -4, "flip_y": sy == -4 * x, "flip_z": sz == -4 * x * y, "flip_all": (sx, sy, sz) == (-4, -4 * x, -4 * x * y),
            "one_row": sy == 0, "one_plane": sz == 0}[kind]
    assert all(o > 0 for o in offsets)                                  # element (0, 0, 0) is not where the file starts
    cases = [(use_d, use_l, r0, r1) for use_d, use_l in ((1, 0), (0, 1), (1, 1)) for r0, r1 in row_ranges(shape)]
    check(views, shape, cases, pack(driver, views, shape, cases, threads, offsets=offsets))
