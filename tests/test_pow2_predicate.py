"""The host predicate that routes a frame to the march's scaled-ray instantiation (csrc/march_pow2.h, svr_ss_pow2): a
per-axis factor size * scale qualifies only as an exact power of two in [1, 2^23].  The header is plain C++; it is
compiled here on its own with the host compiler and asked about each value."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub_volume_renderer_amd", "csrc")

DRIVER = r"""
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "march_pow2.h"
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        uint32_t bits = 0; sscanf(argv[i], "%x", &bits);
        float f; memcpy(&f, &bits, 4);
        putchar(svr_ss_pow2(f) ? '1' : '0');
    }
    putchar('\n');
    return 0;
}
"""


@pytest.fixture(scope="module")
def predicate(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("pow2")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)

    def ask(values):
        bits = [format(int(np.float32(v).view(np.uint32)), "x") for v in values]
        out = subprocess.run([str(exe), *bits], check=True, capture_output=True, text=True).stdout.strip()
        return [c == "1" for c in out]

    return ask


def test_powers_of_two_from_1_to_2_pow_23_qualify(predicate):
    assert all(predicate([2.0 ** k for k in range(24)]))


def test_below_one_never_qualifies(predicate):
    vals = [0.5, 0.25, 2.0 ** -20, 2.0 ** -126, np.float32(2.0 ** -149), 0.0, -0.0]
    assert not any(predicate(vals))


def test_non_powers_of_two_never_qualify(predicate):
    vals = [3.0, 768.0, 250.0, 1023.0, 1025.0, 1.5, np.nextafter(np.float32(1024), np.float32(2048)),
            np.nextafter(np.float32(1024), np.float32(0)), 1024.0 * 0.75, 60.0, 15.0]
    assert not any(predicate(vals))


def test_negative_huge_and_non_finite_never_qualify(predicate):
    vals = [-1.0, -1024.0, 2.0 ** 24, 2.0 ** 100, np.inf, -np.inf, np.nan]
    assert not any(predicate(vals))


def test_benchmark_and_test_extents(predicate):
    """size * 2^-k of the benchmark volumes (1024^3, 2048^3, 4096^3) qualify; C1's 768 and a 250^3 volume do not."""
    good = [n * 2.0 ** -k for n in (1024, 2048, 4096) for k in range(3)]
    assert all(predicate(good))
    assert predicate([768.0, 384.0, 250.0, 125.0]) == [False, False, False, False]
