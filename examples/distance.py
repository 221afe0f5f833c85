#!/usr/bin/env python3
"""The exact Euclidean distance transform (``SubVolume.distance``, ``svr_distance``) on the reference's multi-scale demo
scene (scripts/multi_scale.py).  The level set halfway between the material's contrast limits is labelled on the device
in the finest resident LOD (``SubVolume.components``) and the box of its largest component is taken.  The distance
transform of that box gives the object's radius (its half thickness) and its deepest point: both are printed, and the
windows are centred on the deepest point (``center_on_position(field.deepest_position())``) where
examples/components.py centres on the centroid, which may lie outside a hollow or curved object.  Writes
``distance_object.png``, an iso render cropped to that box, and ``distance_plane.png``, the mid-z plane of
``field.distance()``, white at the deepest.

usage: python examples/distance.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import compose, testing  # noqa: E402

BACKGROUND = ((0.02, 0.02, 0.03, 1.0), (0.10, 0.10, 0.14, 1.0))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.make_multiscale_demo_scene(480, 480)
    volume, camera = scene.volume, scene.camera
    volume.render(camera, scene.width, scene.height)
    lod = next(i for i, b in enumerate(volume.wrapping_buffers) if b._current_logical_roi_in_pixels is not None)

    lo, hi = volume.material.clim
    level = lo + 0.5 * (hi - lo)
    table = volume.components(level=level, lod=lod)
    if not table.count:
        raise SystemExit("the level set is empty")
    largest = table.largest()[0]
    begin, end = table.box(largest)                         # finest scale, numpy order
    print(f"level {level:.6g}, LOD {lod}: {table.count} components; the largest, {largest}, has {int(table.voxels[largest - 1])} voxels "
          f"in the box {begin} .. {end}")

    field = volume.distance(level=level, lod=lod, box=(begin, end))
    print(f"distance transform of a box of {tuple(field.squared.shape)} voxels from {tuple(field.begin)} (z, y, x): {field.targets} voxels inside, "
          f"{field.far_voxels} of them without any outside voxel")
    print(f"  radius {field.radius():.3f} voxels (squared: {field.max_squared}) at the deepest voxel {tuple(field.deepest)}")
    for r in (1, 2, 4):
        print(f"  eroded by {r}: {int(field.eroded(r).sum())} voxels are left")
    outside = volume.distance(level=level, lod=lod, invert=True)      # the whole window: the distance of every outside voxel to the level set
    print(f"  the level set of the window dilated by 2: {outside.inside_voxels} + {int(outside.within(2).sum())} voxels")
    position = field.deepest_position()                     # world (x, y, z)
    centroid = table.position(largest)
    print(f"deepest point {tuple(round(v, 3) for v in position)}: {field.at(position)} squared voxels deep; "
          f"centroid {tuple(round(v, 3) for v in centroid)}: {field.at(centroid)} (0: it lies outside the object)")

    plane = field.distance()[field.squared.shape[0] // 2].cpu().numpy()
    finite = np.where(np.isfinite(plane), plane, 0.0)
    grey = np.round(255.0 * finite / max(float(finite.max()), 1.0)).astype(np.uint8)
    rgba = np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=-1)
    path = os.path.join(out_dir, "distance_plane.png")
    write_png(path, rgba)
    print(f"the mid-z plane of the distances, {plane.shape[1]} x {plane.shape[0]} -> {path}")

    volume.center_on_position(position)
    m = volume.material
    m.render_mode, m.iso_value = "iso", level
    m.cut_planes, m.cut_mode = volume.crop_planes(begin, end), "ANY"
    res = volume.render(camera, scene.width, scene.height)
    path = os.path.join(out_dir, "distance_object.png")
    write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
    print(f"iso cropped to {begin} .. {end}, centred on the deepest point -> {path}  ({int((res.flags == 2).sum())} pixels hit)")


if __name__ == "__main__":
    main()
