"""Seeded differential fuzzing of svr_slice, svr_slab, svr_composite and svr_iso (tools/fuzz_modes.py): the scenes of
the march's fuzzer - 1-4 LODs, anisotropic volumes that are no powers of two, random chunk and ring shapes, rings with no
macro-cell grid, u8 / u16 / f32 data, label-less volumes, windows that moved twice, world scale and translation,
clipping planes, tiles and stripes - with drawn planes, slabs, transfer functions, iso settings, cut planes, sampling and
micro-block copies.  Every plane of every pixel against the numpy twins as tests/test_gpu_linear.py compares them
(discrete planes, the value plane and the slice's depth bit for bit, rgba / depth / normal within its TOL of 1e-4), plus
iso skipping on == off, rows == micro-block copy and slab(max, 1) == slice bit for bit.  Seeds 7064-7183 with perspective
cameras and 7064-7103 with orthographic ones, in blocks of ten (tools/fuzz_modes.SUITE_BLOCKS); tests/test_mode_fuzz.py
holds on the CPU that these seeds exercise every feature of the draw and that the comparison notices perturbed inputs.

One draw is narrowed (``fuzz_modes.bounded_clim``): clim[1] is raised where the volume's largest value would shade to a
colour above 16.  As first drawn, 33 of the 120 perspective and 6 of the 40 orthographic seeds missed 1e-4 on the rgba
plane of the slice and the slab and on nothing else (seed 7132: 0.03125, seed 7179: 134217728.0).  In those scenes the
data ends far above clim[1] (LODs of mixed types keep bytes against a clim of 0 .. 1; clims drawn to end at 100 of 255
under a gamma of 3), the grey chain pow(pow(s, gamma), 2.4) of include/svr.h shades s in the hundreds to colours of
4.6e5 (seed 7132) to 5e14 (seed 7179), and the errors looked at (seeds 7132, 7140, 7179) were one to four float32
spacings of the colour itself: both sides
follow the header's order and differ in the rounding of powf (libm against the device's), which an absolute 1e-4
cannot hold above about 2^10.  The tolerance stays; colours up to 16 hold it with powf good to 16 ulp on either side."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_modes  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("first,ortho", fuzz_modes.SUITE_BLOCKS,
                         ids=[f"{first}{'-ortho' if ortho else ''}" for first, ortho in fuzz_modes.SUITE_BLOCKS])
def test_seeded_random_modes(first, ortho):
    failures = []
    enough = dict.fromkeys(fuzz_modes.ENTRY_POINTS, 0)
    for seed in range(first, first + fuzz_modes.SUITE_BLOCK):
        bad, hits = fuzz_modes.run_case(seed, ortho)
        failures += [f"seed {seed}{' ortho' if ortho else ''}: {entry}: plane {plane}: {figure}" for entry, plane, figure in bad]
        for k in enough:
            enough[k] += hits[k] >= 100
    print("seeds with >= 100 HIT pixels in the twin", enough)
    assert not failures, failures
    assert all(3 * n >= fuzz_modes.SUITE_BLOCK for n in enough.values()), enough
