#!/usr/bin/env python3
"""Segmentation outlines and selected-object highlighting on the reference's multi-scale demo scene
(scripts/multi_scale.py).  Its labels are the level each hit was read from, so the outlines also trace the seams
between levels of detail.  The label under the centre pixel (or the hit nearest to it) is picked, as a cursor
would, and three PNG files are written: the plain frame, the frame with white outlines (the march draws misses
opaque black), and the picked object outlined in its own hue with every other object dimmed.

usage: python examples/outlines.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
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


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.build(testing.multiscale_demo_spec(480, 480))
    volume = scene.volume
    frame = volume.render(scene.camera, scene.width, scene.height)
    grey = lambda v: (v / 255.0,) * 3 + (1.0,)                # noqa: E731
    background = (grey(100), grey(168))                       # bottom, top of the demo's gradient

    hit = (frame.flags == 2).cpu().numpy()
    if not hit.any():
        raise SystemExit("the frame has no hits")
    ys, xs = np.nonzero(hit)
    k = int(np.argmin((ys - scene.height // 2) ** 2 + (xs - scene.width // 2) ** 2))
    picked = int(frame.label_numpy()[ys[k], xs[k]])

    images = {
        "plain": frame,
        "outlined": dataclasses.replace(frame, rgba=outline(volume, frame, width=1, color=(1.0, 1.0, 1.0, 1.0))),
        "selected": dataclasses.replace(frame, rgba=outline(volume, frame, width=2, color_by_label=True, selected=[picked],
                                                            dim_unselected=0.25, only_selected=True)),
    }
    for name, result in images.items():
        path = os.path.join(out_dir, f"outlines_{name}.png")
        write_png(path, compose(volume, result, background=background).cpu().numpy())
        print(f"{name} -> {path}")
    print(f"picked label {picked} at pixel ({xs[k]}, {ys[k]}); {int(hit.sum())} of {hit.size} pixels hit")


if __name__ == "__main__":
    main()
