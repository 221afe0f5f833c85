#!/usr/bin/env python3
"""Cross-section views of the reference's multi-scale demo scene (scripts/multi_scale.py): the three axis-aligned
slices through the point of the volume nearest to the camera, the same slices with their label edges outlined, and
one slice coloured by the level of detail each pixel was read from (the `lod` plane: which scale is resident where).
Writes PNG files.

usage: python examples/slices.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
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

LOD_COLORS = np.array([(230, 80, 60, 255), (70, 170, 90, 255), (60, 110, 220, 255), (200, 190, 60, 255),
                       (160, 80, 200, 255), (60, 190, 200, 255), (220, 140, 60, 255), (140, 140, 140, 255)], np.uint8)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    spec = testing.multiscale_demo_spec(480, 480)
    volume = testing.build(spec).volume
    # the demo's camera stands outside the volume (x < 0): slice through the nearest point inside it instead
    data = (volume.world.inverse_matrix @ np.array([*spec.centers[0][0], 1.0]))[:3]
    data = np.clip(data, 0.0, np.array(volume._volume_dimensions, np.float64) - 1.0)
    focus = tuple((volume.world.matrix @ np.array([*data, 1.0]))[:3])
    width = height = 480
    for axis in ("z", "y", "x"):
        origin, u, v = SubVolume.axis_slice_plane(axis, focus, 0.5)
        s = volume.render_slice(origin, u, v, width, height)
        plain = compose(volume, s)
        outlined = compose(volume, dataclasses.replace(s, rgba=outline(volume, s, width=1, color=(1.0, 1.0, 1.0, 1.0))))
        for name, img in (("plain", plain), ("outlined", outlined)):
            path = os.path.join(out_dir, f"slice_{axis}_{name}.png")
            write_png(path, img.cpu().numpy())
            print(f"{axis}-normal {name} -> {path}  ({int((s.flags == 2).sum())} pixels hit)")
        if axis == "z":
            lod = s.lod.cpu().numpy()
            rgba = np.zeros((height, width, 4), np.uint8)
            rgba[..., 3] = 255
            resident = lod != 255
            rgba[resident] = LOD_COLORS[lod[resident] % len(LOD_COLORS)]
            path = os.path.join(out_dir, "slice_z_lod.png")
            write_png(path, rgba)
            counts = {int(k): int((lod == k).sum()) for k in np.unique(lod)}
            print(f"z-normal by level of detail -> {path}  (pixels per LOD, 255 = not resident / outside: {counts})")
            # the same plane under linear sampling: the 2 x 2 pixel blocks of pixel size 0.5 become gradients
            s = volume.render_slice(origin, u, v, width, height, interpolation="linear")
            path = os.path.join(out_dir, "slice_z_linear.png")
            write_png(path, compose(volume, s).cpu().numpy())
            print(f"z-normal, interpolation='linear' -> {path}")


if __name__ == "__main__":
    main()
