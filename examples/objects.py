#!/usr/bin/env python3
"""Per-object measurements (``SubVolume.objects``, ``svr_objects``) on the reference's multi-scale demo scene
(scripts/multi_scale.py): the scene is rendered, the label under the centre pixel (or the hit nearest to it) is picked
as a cursor would, and its row of the object table of the finest resident LOD is printed - voxels, bounding box,
centroid, mean / min / max.  Then the windows are centred on the object (``center_on_position(table.position(id))``)
and an iso render cropped to ``table.box(id)`` with ``crop_planes`` and outlined with ``selected=[id]`` is written,
beside the plain frame.  Writes two PNG files and ``objects_table.txt`` (every row of the table).

usage: python examples/objects.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import compose, outline, testing  # noqa: E402

BACKGROUND = ((0.02, 0.02, 0.03, 1.0), (0.10, 0.10, 0.14, 1.0))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.make_multiscale_demo_scene(480, 480)
    volume, camera = scene.volume, scene.camera
    frame = volume.render(camera, scene.width, scene.height)
    path = os.path.join(out_dir, "objects_plain.png")
    write_png(path, compose(volume, frame, background=BACKGROUND).cpu().numpy())
    print(f"plain -> {path}")

    hit = (frame.flags == 2).cpu().numpy()
    if not hit.any():
        raise SystemExit("the frame has no hits")
    ys, xs = np.nonzero(hit)
    k = int(np.argmin((ys - scene.height // 2) ** 2 + (xs - scene.width // 2) ** 2))
    picked = int(frame.label_numpy()[ys[k], xs[k]])

    # the finest LOD that holds the picked label
    table = None
    for lod, buffer in enumerate(volume.wrapping_buffers):
        if buffer._current_logical_roi_in_pixels is None:
            continue
        candidate = volume.objects(lod=lod, background=True)
        if picked in candidate.ids.tolist():
            table = candidate
            break
    if table is None:
        raise SystemExit(f"label {picked} is not resident in any LOD")
    rows = {k: getattr(table, k).cpu().numpy() for k in ("ids", "voxels", "begin", "end", "centroid", "finite", "mean", "min", "max")}
    i = table.index(picked)
    print(f"picked label {picked} at pixel ({xs[k]}, {ys[k]}): LOD {table.lod}, {len(table)} objects, {table.considered} voxels")
    print(f"  voxels {rows['voxels'][i]}, box {rows['begin'][i].tolist()} .. {rows['end'][i].tolist()} (z, y, x; LOD voxels), "
          f"centroid {np.round(rows['centroid'][i], 3).tolist()}, mean {rows['mean'][i]:.6g}, min {rows['min'][i]:.6g}, max {rows['max'][i]:.6g}")
    path = os.path.join(out_dir, "objects_table.txt")
    with open(path, "w") as f:
        f.write("# id\tvoxels\tbegin(z,y,x)\tend(z,y,x)\tcentroid(z,y,x)\tmean\tmin\tmax\n")
        for j in range(len(table)):
            f.write(f"{rows['ids'][j]}\t{rows['voxels'][j]}\t{rows['begin'][j].tolist()}\t{rows['end'][j].tolist()}\t"
                    f"{np.round(rows['centroid'][j], 3).tolist()}\t{rows['mean'][j]:.6g}\t{rows['min'][j]:.6g}\t{rows['max'][j]:.6g}\n")
    print(f"{len(table)} rows -> {path}")

    begin, end = table.box(picked)                          # finest scale, numpy order
    position = table.position(picked)                       # world (x, y, z)
    volume.center_on_position(position)
    m = volume.material
    lo, hi = m.clim
    m.render_mode, m.color_by_label = "iso", True
    m.iso_value = lo + 0.5 * (hi - lo)
    m.cut_planes, m.cut_mode = volume.crop_planes(begin, end), "ANY"
    res = volume.render(camera, scene.width, scene.height)
    res = dataclasses.replace(res, rgba=outline(volume, res, width=2, color_by_label=True, selected=[picked], depth_tolerance=0.01))
    path = os.path.join(out_dir, "objects_cropped.png")
    write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
    print(f"iso cropped to {begin} .. {end}, centred on {tuple(round(v, 3) for v in position)} -> {path}  "
          f"({int((res.flags == 2).sum())} pixels hit)")


if __name__ == "__main__":
    main()
