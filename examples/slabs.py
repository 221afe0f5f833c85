#!/usr/bin/env python3
"""Thick-slab projections of the reference's multi-scale demo scene (scripts/multi_scale.py): the z-normal maximum
intensity slab through the point of the volume nearest to the camera at several thicknesses, a mean slab, and a
maximum slab outlined with the depth test (label edges, plus edges where the winning sample jumps in depth).
Writes PNG files.

usage: python examples/slabs.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import SubVolume, compose, outline, testing  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    spec = testing.multiscale_demo_spec(480, 480)
    volume = testing.build(spec).volume
    # the demo's camera stands outside the volume (x < 0): centre the slabs on the nearest point inside it instead
    data = (volume.world.inverse_matrix @ np.array([*spec.centers[0][0], 1.0]))[:3]
    data = np.clip(data, 0.0, np.array(volume._volume_dimensions, np.float64) - 1.0)
    focus = tuple((volume.world.matrix @ np.array([*data, 1.0]))[:3])
    width = height = 480
    origin, u, v, w = SubVolume.axis_slab_plane("z", focus, 0.5, 0.5)
    for samples in (1, 8, 32):
        s = volume.render_slab(origin, u, v, w, samples, width, height, mode="max")
        path = os.path.join(out_dir, f"slab_z_max_{samples}.png")
        write_png(path, compose(volume, s).cpu().numpy())
        print(f"z-normal max slab of {samples} samples -> {path}  ({int((s.flags == 2).sum())} pixels hit)")
    s = volume.render_slab(origin, u, v, w, 32, width, height, mode="mean")
    path = os.path.join(out_dir, "slab_z_mean_32.png")
    write_png(path, compose(volume, s).cpu().numpy())
    print(f"z-normal mean slab of 32 samples -> {path}")
    s = volume.render_slab(origin, u, v, w, 32, width, height, mode="max")
    edges = outline(volume, s, width=1, color=(1.0, 1.0, 1.0, 1.0), depth_tolerance=2.0)
    path = os.path.join(out_dir, "slab_z_max_32_outlined.png")
    write_png(path, compose(volume, dataclasses.replace(s, rgba=edges)).cpu().numpy())
    print(f"z-normal max slab of 32 samples, outlined with a depth tolerance of 2 -> {path}")


if __name__ == "__main__":
    main()
