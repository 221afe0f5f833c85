#!/usr/bin/env python3
"""Intensity histogram and automatic contrast limits of the reference's multi-scale demo scene
(scripts/multi_scale.py): the scene rendered with its default ``clim`` and with the pair ``auto_clim()`` proposes from
what is resident in HBM, and the histogram of every LOD that has a window written as text.  Writes two PNG files and
``histogram_counts.txt``.

usage: python examples/histogram.py [out_dir]        (needs an MI355X and the built libsvr_hip.so)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from multi_scale import write_png  # noqa: E402
from sub_volume_renderer_amd import compose, testing  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    scene = testing.build(testing.multiscale_demo_spec(480, 480))
    volume = scene.volume
    path = os.path.join(out_dir, "histogram_default_clim.png")
    write_png(path, compose(volume, volume.render(scene.camera, 480, 480)).cpu().numpy())
    print(f"clim {volume.material.clim} (the material's) -> {path}")

    lines = []
    for lod, buffer in enumerate(volume.wrapping_buffers):
        if buffer._current_logical_roi_in_pixels is None:
            continue
        h = volume.histogram(lod=lod, bins=16)          # float32 rings: the range is the resident minimum .. maximum
        counts = h.counts.cpu().numpy()
        lines.append(f"# LOD {lod}: {h.considered} voxels, min {h.min}, max {h.max}, under {h.under}, over {h.over}, NaN {h.nan}")
        lines += [f"{h.edges[j]:.6g}\t{h.edges[j + 1]:.6g}\t{int(c)}" for j, c in enumerate(counts)]
    path = os.path.join(out_dir, "histogram_counts.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} lines -> {path}")

    low, high = volume.auto_clim((0.5, 99.5))           # from the coarsest LOD that has a window
    volume.material.clim = (low, high)
    path = os.path.join(out_dir, "histogram_auto_clim.png")
    write_png(path, compose(volume, volume.render(scene.camera, 480, 480)).cpu().numpy())
    print(f"clim ({low}, {high}) (auto_clim) -> {path}")


if __name__ == "__main__":
    main()
