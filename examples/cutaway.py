#!/usr/bin/env python3
"""Cut-away views (``SubVolumeMaterial.cut_planes``, ``svr_set_cut_planes``) of the reference's multi-scale demo scene
(scripts/multi_scale.py), from its own camera:
  cutaway_iso_wedge           the iso-surface with the octant towards the camera removed from the nearest blocks (three
                              planes, cut_mode "ALL"): the cut faces are flat, lit caps;
  cutaway_iso_wedge_by_label  the same coloured by the segmentation labels and outlined;
  cutaway_composite_half      direct volume rendering with everything in front of one plane removed (cut_mode "ANY");
  cutaway_iso_crop            the iso-surface cropped to a voxel box with ``SubVolume.crop_planes``.
Each frame is composed over a dark background.  Writes PNG files.

usage: python examples/cutaway.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import TransferFunction, compose, outline, testing  # noqa: E402

BACKGROUND = ((0.02, 0.02, 0.03, 1.0), (0.10, 0.10, 0.14, 1.0))


def wedge_towards(eye, focus):
    """The three axis planes through ``focus`` whose common back side is the octant that holds ``eye``."""
    planes = []
    for a in range(3):
        s = 1.0 if eye[a] >= focus[a] else -1.0
        n = [0.0, 0.0, 0.0]
        n[a] = -s
        planes.append((*n, -s * focus[a]))
    return planes


def half_towards(eye, through):
    """The plane through ``through`` that faces ``eye``: what lies on the eye's side of it is behind it."""
    n = np.asarray(through, float) - np.asarray(eye, float)
    n = n / np.linalg.norm(n)
    return [(*n, float(n @ np.asarray(through, float)))]


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.make_multiscale_demo_scene(480, 480)
    volume, camera = scene.volume, scene.camera
    eye = scene.spec.cam_position
    m = volume.material
    lo, hi = m.clim
    m.iso_value, m.iso_color, m.light_direction = lo + 0.5 * (hi - lo), (0.85, 0.75, 0.6), (-0.5, 0.7, 0.5)
    m.transfer_function = TransferFunction.linear(color=(0.9, 0.8, 0.6), opacity=0.6)
    views = [
        # the demo's blocks are 4^3 voxels at the chunk corners: a wedge through the middle of the nearest ones
        ("iso_wedge", "iso", wedge_towards(eye, (1.5, 1.5, 1.5)), "ALL", False),
        ("iso_wedge_by_label", "iso", wedge_towards(eye, (1.5, 1.5, 1.5)), "ALL", True),
        ("composite_half", "composite", half_towards(eye, (1.5, 4.0, 4.0)), "ANY", False),
        ("iso_crop", "iso", volume.crop_planes((0, 0, 0), (40, 40, 100)), "ANY", False),
    ]
    for name, mode, planes, cut_mode, by_label in views:
        m.render_mode, m.cut_planes, m.cut_mode, m.color_by_label = mode, planes, cut_mode, by_label
        res = volume.render(camera, scene.width, scene.height)
        if by_label:
            res = dataclasses.replace(res, rgba=outline(volume, res, width=1, depth_tolerance=0.01))
        path = os.path.join(out_dir, f"cutaway_{name}.png")
        write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
        print(f"{name}: {mode}, {len(planes)} planes, cut_mode {cut_mode} -> {path}  ({int((res.flags == 2).sum())} pixels hit)")


if __name__ == "__main__":
    main()
