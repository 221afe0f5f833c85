#!/usr/bin/env python3
"""Surface meshes (``SubVolume.mesh``, ``svr_mesh``) on the reference's multi-scale demo scene (scripts/multi_scale.py):
the scene is rendered, the label under the centre pixel (or the hit nearest to it) is picked as a cursor would, and the
picked object of the finest LOD that holds it is extracted on the device as a closed triangle mesh and written as a
Wavefront OBJ file in world coordinates.  Then one level set of the same LOD (the level halfway between the material's
contrast limits) is written the same way.  Prints vertices, triangles, surface area and enclosed volume of both.

usage: python examples/mesh.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from sub_volume_renderer_amd import testing  # noqa: E402


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

    mesh = None
    for lod, buffer in enumerate(volume.wrapping_buffers):             # the finest LOD that holds the picked label
        if buffer._current_logical_roi_in_pixels is None:
            continue
        candidate = volume.mesh(labels=[picked], lod=lod)
        if len(candidate):
            mesh = candidate
            break
    if mesh is None:
        raise SystemExit(f"label {picked} is not resident in any LOD")
    path = os.path.join(out_dir, "mesh_object.obj")
    mesh.write_obj(path)
    print(f"label {picked} at pixel ({xs[k]}, {ys[k]}), LOD {mesh.lod}: V {mesh.vertices.shape[0]}, T {len(mesh)}, "
          f"{mesh.inside_voxels} voxels, area {mesh.area():.6g}, volume {mesh.enclosed_volume():.6g} -> {path}")

    lo, hi = volume.material.clim
    level = lo + 0.5 * (hi - lo)
    surface = volume.mesh(level=level, lod=mesh.lod)
    path = os.path.join(out_dir, "mesh_level.obj")
    surface.write_obj(path)
    print(f"level {level:.6g}, LOD {surface.lod}: V {surface.vertices.shape[0]}, T {len(surface)}, {surface.inside_voxels} voxels, "
          f"area {surface.area():.6g}, volume {surface.enclosed_volume():.6g} -> {path}")
    if not (mesh.enclosed_volume() > 0 and surface.enclosed_volume() > 0):
        raise SystemExit("a mesh encloses no volume")


if __name__ == "__main__":
    main()
