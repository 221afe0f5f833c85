#!/usr/bin/env python3
"""Connected components (``SubVolume.components``, ``svr_components``) on the reference's multi-scale demo scene
(scripts/multi_scale.py).  The level set halfway between the material's contrast limits is labelled on the device in the
finest resident LOD: the number of blobs and the five largest are printed, the windows are centred on the largest
(``center_on_position(table.position(id))``) and an iso render cropped to ``table.box(id)`` with ``crop_planes`` is
written.  Then the object under the centre pixel is picked as a cursor would pick it, and the number of pieces its label
lies in is printed.  Writes ``components_largest.png`` and ``components_table.txt`` (every row of the level set's table).

usage: python examples/components.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
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
    frame = volume.render(camera, scene.width, scene.height)
    hit = (frame.flags == 2).cpu().numpy()
    if not hit.any():
        raise SystemExit("the frame has no hits")
    ys, xs = np.nonzero(hit)
    k = int(np.argmin((ys - scene.height // 2) ** 2 + (xs - scene.width // 2) ** 2))
    picked = int(frame.label_numpy()[ys[k], xs[k]])
    lod = next(i for i, b in enumerate(volume.wrapping_buffers) if b._current_logical_roi_in_pixels is not None)

    # unsegmented data: the blobs of a level set
    lo, hi = volume.material.clim
    level = lo + 0.5 * (hi - lo)
    table = volume.components(level=level, lod=lod)
    print(f"level {level:.6g}, LOD {lod}: {table.count} components, {table.inside_voxels} voxels inside, box of {tuple(table.ids.shape)} voxels "
          f"from {tuple(table.begin)} (z, y, x)")
    if not table.count:
        raise SystemExit("the level set is empty")
    rows = {name: getattr(table, name).cpu().numpy() for name in ("voxels", "first", "lo", "end", "centroid")}
    for number in table.largest(5):
        i = number - 1
        print(f"  component {number}: {rows['voxels'][i]} voxels, box {rows['lo'][i].tolist()} .. {rows['end'][i].tolist()}, "
              f"centroid {np.round(rows['centroid'][i], 3).tolist()}")
    path = os.path.join(out_dir, "components_table.txt")
    with open(path, "w") as f:
        f.write("# id\tvoxels\tfirst(z,y,x)\tlo(z,y,x)\tend(z,y,x)\tcentroid(z,y,x)\n")
        for i in range(table.count):
            f.write(f"{i + 1}\t{rows['voxels'][i]}\t{rows['first'][i].tolist()}\t{rows['lo'][i].tolist()}\t{rows['end'][i].tolist()}\t"
                    f"{np.round(rows['centroid'][i], 3).tolist()}\n")
    print(f"{table.count} rows -> {path}")

    # segmented data: is the picked object one piece?  (asked before the windows move)
    pieces = None
    for plod, buffer in enumerate(volume.wrapping_buffers):            # the finest LOD that holds the picked label
        if buffer._current_logical_roi_in_pixels is None:
            continue
        candidate = volume.components(labels=[picked], background=True, lod=plod)
        if candidate.count:
            pieces = candidate
            break

    largest = table.largest()[0]
    begin, end = table.box(largest)                         # finest scale, numpy order
    position = table.position(largest)                      # world (x, y, z)
    print(f"component under the centroid of component {largest}: {table.id_at(position)} (0: the centroid lies outside the level set)")
    volume.center_on_position(position)
    m = volume.material
    m.render_mode, m.iso_value = "iso", level
    m.cut_planes, m.cut_mode = volume.crop_planes(begin, end), "ANY"
    res = volume.render(camera, scene.width, scene.height)
    path = os.path.join(out_dir, "components_largest.png")
    write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
    print(f"iso cropped to component {largest}, {begin} .. {end}, centred on {tuple(round(v, 3) for v in position)} -> {path}  "
          f"({int((res.flags == 2).sum())} pixels hit)")

    if pieces is None:
        raise SystemExit(f"label {picked} is not resident in any LOD")
    sizes = pieces.voxels.cpu().numpy()
    print(f"picked label {picked} at pixel ({xs[k]}, {ys[k]}), LOD {pieces.lod}: {len(pieces.pieces(picked))} pieces, "
          f"the largest of {int(sizes.max())} voxels, {int(sizes.sum())} voxels in all")


if __name__ == "__main__":
    main()
