#!/usr/bin/env python3
"""Direct volume rendering (the composite render mode, ``svr_composite``) of the reference's multi-scale demo scene
(scripts/multi_scale.py), from its own camera: a faint grey transfer function that shows every layer, a coloured
piecewise-linear one that turns opaque on the dense blocks, and the same one tinted by the segmentation labels.  Each
frame is composed over a dark background.  Writes PNG files.

usage: python examples/composite.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import TransferFunction, compose, testing  # noqa: E402

BACKGROUND = ((0.02, 0.02, 0.03, 1.0), (0.10, 0.10, 0.14, 1.0))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.make_multiscale_demo_scene(480, 480)
    volume, camera = scene.volume, scene.camera
    m = volume.material
    m.render_mode = "composite"
    warm = TransferFunction.from_points([(0.0, (0.1, 0.2, 0.6, 0.0)), (0.5, (0.9, 0.5, 0.2, 0.3)), (1.0, (1.0, 0.95, 0.8, 0.9))])
    views = [
        ("faint", TransferFunction.linear(color=(0.8, 0.8, 0.8), opacity=0.15), 1.0, False),
        ("warm", warm, 0.99, False),
        ("by_label", TransferFunction.linear(opacity=0.6), 0.99, True),
    ]
    for name, tf, cutoff, tint in views + [("warm_linear", warm, 0.99, False)]:
        m.interpolation = "linear" if name.endswith("_linear") else "nearest"     # the ray's input: eight texels blended
        m.transfer_function, m.alpha_cutoff, m.color_by_label = tf, cutoff, tint
        res = volume.render(camera, scene.width, scene.height, count_steps=True)
        path = os.path.join(out_dir, f"composite_{name}.png")
        write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
        hit = int((res.flags == 2).sum())
        print(f"{name}: cutoff {cutoff}, tinted by label: {tint} -> {path}  ({hit} pixels hit, "
              f"{int(res.steps.sum())} samples visited)")


if __name__ == "__main__":
    main()
