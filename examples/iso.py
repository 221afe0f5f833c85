#!/usr/bin/env python3
"""Lit iso-surfaces (the iso render mode, ``svr_iso``) of the reference's multi-scale demo scene
(scripts/multi_scale.py), from its own camera, at two levels: a low one under the headlight, and a higher one coloured
by the segmentation labels, lit from the upper left and outlined.  (The demo's field is 0 / 1, so both levels find
the same blocks; real data separates them.)  Each frame is composed over a dark background.  Writes PNG files.

usage: python examples/iso.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import dataclasses
import os
import sys

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
    m = volume.material
    m.render_mode = "iso"
    lo, hi = m.clim
    views = [
        ("low", lo + 0.25 * (hi - lo), dict(color_by_label=False, iso_color=(0.85, 0.75, 0.6), light_direction=None)),
        ("by_label", lo + 0.5 * (hi - lo), dict(color_by_label=True, light_direction=(-0.5, 0.7, 0.5), specular=0.5)),
    ]
    # the last view again under linear sampling: smooth surfaces and normals instead of voxel staircases
    views.append(("by_label_linear", views[-1][1], dict(views[-1][2], interpolation="linear")))
    for name, level, settings in views:
        m.iso_value = level
        for key, value in settings.items():
            setattr(m, key, value)
        out = volume.iso_outputs(scene.width, scene.height, count_steps=True, skip_counters=True)
        res = volume.render(camera, scene.width, scene.height, count_steps=True, out=out)
        if m.color_by_label:
            res = dataclasses.replace(res, rgba=outline(volume, res, width=1, depth_tolerance=0.01))
        path = os.path.join(out_dir, f"iso_{name}.png")
        write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
        marched, skipped = (int(v) for v in out.skip_counters.cpu().numpy())
        print(f"{name}: level {level:g}, coloured by label: {m.color_by_label} -> {path}  ({int((res.flags == 2).sum())} "
              f"pixels hit, {int(out.steps.sum())} coarse samples, {skipped} of {marched + skipped} wave-stretches skipped)")


if __name__ == "__main__":
    main()
