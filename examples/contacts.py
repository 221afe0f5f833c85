#!/usr/bin/env python3
"""Contacts between objects (``SubVolume.contacts``, ``svr_contacts``) on the reference's multi-scale demo scene
(scripts/multi_scale.py) and, because that scene has one label per LOD and so no contact at all, on the synthetic
three-LOD scene of the benchmark at 64^3: the scene is rendered, the labelled object under the centre pixel (or the one nearest to it) is
picked as a cursor would, and the five neighbours it touches over the most faces (label 0, the unlabelled rest, among them) are printed with their contact areas and the
mean value along each contact, beside its free surface (its contact with label 0) and its whole surface.  Then the
windows are centred on the largest contact (``center_on_position(table.position(a, b))``) and an iso render cropped to
``table.box(a, b)``, one voxel wider so that both sides of the faces show, and outlined with ``selected=(a, b)`` is
written beside the plain frame.  Writes two PNG files.

usage: python examples/contacts.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
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
    # the demo scene's segmentation is one label per LOD: nothing touches anything there, which the call reports as an
    # empty table; the synthetic three-LOD scene of the benchmark, shrunk to 64^3, has objects that touch
    for name, build in (("the demo scene", lambda: testing.make_multiscale_demo_scene(480, 480)),
                        ("the synthetic scene", lambda: testing.build(testing.synthetic_spec(64, 480, 480)))):
        scene = build()
        if contacts_of(scene, name, out_dir):
            return
        scene.volume.close()
    raise SystemExit("no scene with a contact")


def contacts_of(scene, name, out_dir):
    """Picks, lists, centres and crops on one scene -> False when the picked object touches nothing."""
    volume, camera = scene.volume, scene.camera
    frame = volume.render(camera, scene.width, scene.height)
    hit = (frame.flags == 2).cpu().numpy() & (frame.label_numpy() != 0)      # an object, not the unlabelled rest
    if not hit.any():
        print(f"{name}: the frame has no hit on a labelled object")
        return False
    ys, xs = np.nonzero(hit)
    k = int(np.argmin((ys - scene.height // 2) ** 2 + (xs - scene.width // 2) ** 2))
    picked = int(frame.label_numpy()[ys[k], xs[k]])

    # the finest LOD in which the picked object touches another object; else the finest one that holds it at all (in the
    # demo scene the objects lie apart, and what an object touches is the unlabelled rest, label 0: its free surface)
    table = None
    for wanted in ("an object", "anything"):
        for lod, buffer in enumerate(volume.wrapping_buffers):
            if buffer._current_logical_roi_in_pixels is None or table is not None:
                continue
            candidate = volume.contacts(lod=lod, labels=[picked], background=True)
            partners = candidate.neighbours(picked)[0]
            if len(partners) and (wanted == "anything" or any(int(i) != 0 for i in partners)):
                table = candidate
    if table is None:
        print(f"{name}: label {picked} under pixel ({xs[k]}, {ys[k]}) has no face with another label in any LOD")
        return False
    path = os.path.join(out_dir, "contacts_plain.png")
    write_png(path, compose(volume, frame, background=BACKGROUND).cpu().numpy())
    print(f"{name}: plain -> {path}")
    ids, areas = table.neighbours(picked)
    mean, data_area = table.mean.cpu().numpy(), table.data_area().cpu().numpy()
    free = int(areas[ids == 0].sum())
    print(f"picked label {picked} at pixel ({xs[k]}, {ys[k]}): LOD {table.lod}, {table.voxels} voxels searched, {len(table)} contacts, "
          f"surface {table.surface(picked)} faces of which {free} are free (label 0)")
    for other, area in list(zip(ids.tolist(), areas.tolist()))[:5]:
        row = table.index(picked, other)
        print(f"  touches {other}{' (unlabelled)' if other == 0 else ''}: {area} faces, {data_area[row]:.6g} finest voxels^2, "
              f"mean value along the contact {mean[row]:.6g}")

    a, b = sorted((picked, int(ids[0])))                    # the largest contact
    begin, end = table.box(a, b)                            # finest scale, numpy order: the owning voxels
    pad = tuple(int(np.ceil(1.0 / s)) for s in table.scale_factor)
    begin, end = tuple(v - p for v, p in zip(begin, pad)), tuple(v + p for v, p in zip(end, pad))
    position = table.position(a, b)                         # world (x, y, z)
    volume.center_on_position(position)
    m = volume.material
    lo, hi = m.clim
    m.render_mode, m.color_by_label = "iso", True
    m.iso_value = lo + 0.5 * (hi - lo)
    m.cut_planes, m.cut_mode = volume.crop_planes(begin, end), "ANY"
    res = volume.render(camera, scene.width, scene.height)
    res = dataclasses.replace(res, rgba=outline(volume, res, width=2, color_by_label=True, selected=[v for v in (a, b) if v != 0], depth_tolerance=0.01))
    path = os.path.join(out_dir, "contacts_cropped.png")
    write_png(path, compose(volume, res, background=BACKGROUND).cpu().numpy())
    print(f"largest contact ({a}, {b}): iso cropped to {begin} .. {end}, centred on {tuple(round(v, 3) for v in position)} -> {path}  "
          f"({int((res.flags == 2).sum())} pixels hit)")
    return True


if __name__ == "__main__":
    main()
