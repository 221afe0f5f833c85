#!/usr/bin/env python3
"""Touching objects split apart (``SubVolume.split``, ``svr_split``) on the reference's multi-scale demo scene
(scripts/multi_scale.py).  The level set halfway between the material's contrast limits is labelled on the device in the
finest resident LOD (``SubVolume.components``) and the box of its largest component is taken: one blob that is really
many objects that touch.  The watershed of that box's distance transform cuts it into regions, one per deepest point that
stands more than ``merge`` voxels above the passes around it; the five largest are printed with their radii, the windows
are centred on the deepest point of the largest (``center_on_position(regions.position(id))``), and
``split_object.png``, an iso render cropped to that region's box, is written beside ``split_plane.png``, the region
numbers on the z plane through that point.

usage: python examples/split.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
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
    table = volume.components(level=level, lod=lod, connectivity=26)
    if not table.count:
        raise SystemExit("the level set is empty")
    blob = table.largest()[0]
    begin, end = table.box(blob)                            # finest scale, numpy order
    print(f"level {level:.6g}, LOD {lod}: {table.count} components; the largest, {blob}, has {int(table.voxels[blob - 1])} voxels "
          f"in the box {begin} .. {end}")

    field = volume.distance(level=level, lod=lod, box=(begin, end))
    for merge in (0.0, 1.0, 2.0):
        regions = volume.split(distance=field, merge=merge)
        print(f"  merge {merge:g}: {regions.basins} summits -> {regions.count} regions")
    regions = volume.split(distance=field, merge=1.0)
    if not regions.count:
        raise SystemExit("nothing to split")
    print(f"the five largest of the {regions.count} regions (merge 1, 26-connectivity):")
    for k in regions.largest(5):
        print(f"  region {k}: {int(regions.voxels[k - 1])} voxels, {int(regions.region_basins[k - 1])} summits, radius {regions.radius(k):.3f} voxels "
              f"at {tuple(int(v) for v in regions.top[k - 1])} (z, y, x), box {regions.box(k)}")
    first = regions.largest(1)[0]
    position = regions.position(first)                      # world (x, y, z) of its deepest point
    assert regions.id_at(position) == first

    top = regions.top[first - 1]
    plane = regions.ids[int(top[0]) - regions.begin[0]].cpu().numpy()
    colours = np.random.default_rng(1).integers(64, 256, (regions.count + 1, 3)).astype(np.uint8)
    colours[0] = 0
    rgba = np.concatenate([colours[plane], np.full(plane.shape + (1,), 255, np.uint8)], axis=-1)
    path = os.path.join(out_dir, "split_plane.png")
    write_png(path, rgba)
    print(f"the region numbers on the z plane through the deepest point of region {first}, {plane.shape[1]} x {plane.shape[0]} -> {path}")

    region_begin, region_end = regions.box(first)
    volume.center_on_position(position)
    m = volume.material
    m.render_mode, m.iso_value = "iso", level
    m.cut_planes, m.cut_mode = volume.crop_planes(region_begin, region_end), "ANY"
    res = volume.render(camera, scene.width, scene.height)
    path = os.path.join(out_dir, "split_object.png")
    write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
    print(f"iso cropped to {region_begin} .. {region_end}, centred on {tuple(round(v, 3) for v in position)} -> {path}  "
          f"({int((res.flags == 2).sum())} pixels hit)")


if __name__ == "__main__":
    main()
