#!/usr/bin/env python3
"""The nearest source of every voxel (``SubVolume.nearest``, ``svr_nearest``) and label growth
(``SubVolume.expand_labels``) on the synthetic three-LOD scene of the benchmark at 64^3, whose objects touch one another
(the demo scene of scripts/multi_scale.py has one label per LOD).  The scene is rendered and the labelled object under the
centre pixel (or the one nearest to it) is picked as a cursor would; it and the objects it touches
(``SubVolume.contacts``) are grown by R voxels without merging them, every grown voxel taking the label of the nearest
object, and the voxels each gained are printed.  Then the object's centroid, the "picked position", is snapped to the
surface: from inside the object to the nearest voxel that is not part of it, from outside to the nearest voxel of it
(``NearestField.nearest_position``), and the windows are centred there.  Writes ``nearest_grown.png``, the mid-z plane of
the grown labels, a colour per label.

usage: python examples/nearest.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import testing  # noqa: E402

R = 3.0


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.build(testing.synthetic_spec(64, 480, 480))
    volume, camera = scene.volume, scene.camera
    frame = volume.render(camera, scene.width, scene.height)
    hit = (frame.flags == 2).cpu().numpy() & (frame.label_numpy() != 0)      # an object, not the unlabelled rest
    if not hit.any():
        raise SystemExit("the frame has no hit on a labelled object")
    ys, xs = np.nonzero(hit)
    k = int(np.argmin((ys - scene.height // 2) ** 2 + (xs - scene.width // 2) ** 2))
    picked = int(frame.label_numpy()[ys[k], xs[k]])
    lod = next(i for i, b in enumerate(volume.wrapping_buffers) if b._current_logical_roi_in_pixels is not None)

    partners = [int(i) for i in volume.contacts(lod=lod, labels=[picked], background=True).neighbours(picked)[0] if int(i) != 0]
    group = [picked, *partners]
    print(f"picked label {picked} at pixel ({xs[k]}, {ys[k]}), LOD {lod}; it touches {partners if partners else 'no other object'}")

    field = volume.nearest(labels=group, invert=True, lod=lod)          # the sources are the voxels of the group
    grown = field.expanded(R)
    same = volume.expand_labels(R, labels=group, lod=lod)
    assert np.array_equal(grown.cpu().numpy(), same.cpu().numpy())
    print(f"nearest source of {field.targets} voxels outside the group in a window of {tuple(field.squared.shape)} voxels (z, y, x); "
          f"the farthest lies {field.radius():.3f} voxels from its object, {field.far_voxels} have none")
    before, after = field.expanded(0).cpu().numpy(), grown.cpu().numpy()
    for label in group:
        b, a = int((before == label).sum()), int((after == label).sum())
        print(f"  label {label}: {b} voxels, grown by {R:g}: {a} (+{a - b})")
    print(f"  in all {int((after != 0).sum()) - int((before != 0).sum())} voxels gained; no voxel changed its label: "
          f"{bool(((before == 0) | (before == after)).all())}")

    position = volume.objects(lod=lod, labels=[picked]).position(picked)  # world (x, y, z): the picked position
    inner = volume.nearest(labels=[picked], lod=lod)                    # from inside: the nearest voxel that is not the object
    depth = inner.at(position)
    if depth > 0:
        snapped, how = inner.nearest_position(position), f"{np.sqrt(depth):.3f} voxels inside the object: the nearest voxel outside it"
    else:
        outer = volume.nearest(labels=[picked], invert=True, lod=lod)
        snapped, how = outer.nearest_position(position), f"{np.sqrt(outer.at(position)):.3f} voxels outside the object: the nearest voxel of it"
    print(f"centroid {tuple(round(v, 3) for v in position)} lies {how}, at {tuple(round(v, 3) for v in snapped)}")
    volume.center_on_position(snapped)
    print("windows centred on the snapped position")

    plane = after[after.shape[0] // 2]
    rgba = np.zeros((*plane.shape, 4), np.uint8)
    rgba[..., 3] = 255
    for label in np.unique(plane[plane != 0]):
        rng = np.random.default_rng(int(label))
        rgba[plane == label, :3] = rng.integers(64, 256, 3)
    was = before[before.shape[0] // 2]
    rgba[(plane != 0) & (was == 0), :3] //= 2                           # the gained voxels, darker
    path = os.path.join(out_dir, "nearest_grown.png")
    write_png(path, rgba)
    print(f"the mid-z plane of the grown labels, {plane.shape[1]} x {plane.shape[0]} -> {path}")


if __name__ == "__main__":
    main()
