"""The exact Euclidean distance transform of what a LOD holds in HBM: ``SubVolume.distance`` over ``svr_distance``
(include/svr.h), which takes the squared distance of every inside voxel of a level set (``level``) or of the
segmentation's objects to the nearest voxel that is not inside, on the device, and :class:`DistanceField`, which carries
the dense volume of squared distances, its largest value and where that lies."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._box_pass import box_pass, level32
from ._wobject import label_ids, lod_center_to_world

__all__ = ["DistanceField", "distance", "distance_arguments", "signed_squared"]

FAR = N.DISTANCE_FAR


@dataclass
class DistanceField:
    """The result of one ``SubVolume.distance`` call.  ``squared`` holds squared distances in voxels of the LOD: a
    positive value at a target (an inside voxel; with ``invert=True`` a voxel that is not inside), 0 elsewhere, ``FAR``
    (0x7FFFFFFF) at a target that has no source at all; a ``signed=True`` field is negative outside and ``-FAR`` there.
    Coordinates are LOD voxels in numpy order (z, y, x)."""

    squared: "object"         # torch i32 [n_z, n_y, n_x]; voxel [0, 0, 0] is ``begin``
    begin: tuple              # the first voxel of the box (box and window intersected)
    offset: tuple             # the window offset of the LOD
    inside_voxels: int
    targets: int              # the voxels that have a distance: inside_voxels, or the others with invert=True
    far_voxels: int           # the targets whose distance is FAR
    max_squared: int          # the largest squared distance of a target that is not FAR, 0 if there is none
    deepest: tuple            # the first voxel, in (z, y, x) order, that attains it; ``begin`` if there is none
    lod: int
    background: int = 0       # label-0 voxels left out by background=False
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform

    def distance(self):
        """The distances themselves as float32 in LOD voxels, on the device: the square root of ``squared`` (with its
        sign on a signed field), ``FAR`` as infinity."""
        import torch

        mag = self.squared.abs()
        root = torch.sqrt(mag.to(torch.float64)).to(torch.float32)
        root = torch.where(mag == FAR, torch.full_like(root, float("inf")), root)
        return torch.where(self.squared < 0, -root, root)

    def radius(self) -> float:
        """The largest distance of a target: the radius of the largest ball around ``deepest`` that holds no source."""
        return float(np.sqrt(float(self.max_squared)))

    def deepest_position(self):
        """The world-space position (x, y, z) of ``deepest``, for :meth:`SubVolume.center_on_position`: the arithmetic
        of ``ComponentLabels.position`` on the centre of that voxel."""
        return lod_center_to_world(self.volume, np.asarray(self.deepest, np.float64), self.scale_factor)

    def eroded(self, r):
        """The targets that lie more than ``r`` voxels from every source, as a bool tensor of ``squared``'s shape on the
        device: the erosion of the target set by a ball of radius ``r``.  A ``FAR`` target is in it whatever ``r``."""
        return self.squared > _square(r)

    def within(self, r):
        """The targets that lie at most ``r`` voxels from a source.  On an ``invert=True`` field, ``within(r)`` OR-ed
        with the inside set is the dilation of the inside set by a ball of radius ``r``."""
        return (self.squared > 0) & (self.squared <= _square(r))

    def at(self, position) -> int:
        """The squared distance of the voxel that holds the world-space ``position`` (x, y, z), 0 outside the box: the
        depth under a picked point."""
        voxel = self._voxel(position)
        return 0 if voxel is None else int(self.squared[voxel])

    def _voxel(self, position):
        """The voxel of the box (z, y, x, from ``begin``) that holds the world-space ``position``, None outside the box."""
        world = np.array([float(v) for v in position] + [1.0], np.float64)
        data = (np.linalg.inv(np.asarray(self.volume.world.matrix, np.float64)) @ world)[:3][::-1]          # numpy order
        # the LOD voxel that holds finest data coordinate d: the inverse of lod_center_to_data, rounded to the voxel
        voxel = np.floor((data + 0.5) * np.asarray(self.scale_factor, np.float64)).astype(np.int64) - np.asarray(self.begin, np.int64)
        if np.any(voxel < 0) or np.any(voxel >= np.asarray(tuple(self.squared.shape), np.int64)):
            return None
        return int(voxel[0]), int(voxel[1]), int(voxel[2])


def _square(r) -> int:
    """floor(r^2), which compares with an integer d2 as r^2 does, kept below FAR: no finite r reaches a FAR target."""
    if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, float, np.integer, np.floating)) or not r >= 0:
        raise ValueError("distance: r must be a number >= 0")
    return int(min(np.floor(float(r) * float(r)), FAR - 1))


def signed_squared(inside, outside):
    """The ``signed=True`` combination of the two calls' int32 tensors: d2(invert=0) - d2(invert=1).  At every voxel at
    most one of the two is not 0, so nothing is mixed; a ``FAR`` of the first stays ``FAR`` and a ``FAR`` of the second
    becomes ``-FAR``."""
    return inside - outside


def distance_arguments(level, labels, background, invert, border, signed):
    """What ``SubVolume.distance`` checks before it touches the device -> ``(mode, ids, level, ignore_zero, invert,
    border, signed)``: ``level`` (a number that is not NaN in float32) and ``labels`` exclude one another, the three
    switches are bools; anything else is a ``ValueError``."""
    for name, v in (("invert", invert), ("border", border), ("signed", signed)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"distance: {name} must be True or False")
    if level is not None and labels is not None:
        raise ValueError("distance: give level= or labels=, not both")
    switches = (1 if invert else 0, 1 if border else 0, bool(signed))
    if level is None:
        ids = label_ids(labels) if labels is not None else None
        return (N.COMPONENTS_LABELS, ids, 0.0, 0 if background else 1, *switches)
    return (N.COMPONENTS_LEVEL, None, level32("distance", level), 0, *switches)


def distance(volume, level=None, labels=None, background=False, invert=False, border=True, signed=False, lod: int = 0, box=None,
             stream=None) -> DistanceField:
    """``SubVolume.distance``: see there."""
    import torch

    dp = N.DistanceParams()
    dp.mode, ids, dp.level, dp.ignore_zero, invert, dp.border, signed = distance_arguments(level, labels, background, invert, border, signed)
    lod, scale, dev, c_call = box_pass(volume, "svr_distance", dp, lod, box, ids, stream)

    def call(dense):
        do = lambda header: N.DistanceOutputs(None if dense is None else dense.data_ptr(), 0 if dense is None else dense.numel(), header)
        return c_call(16, do, dense)

    def run(inverted):
        dp.invert = inverted
        head = call(None)                                              # count ...
        while True:
            shape = (head[12], head[11], head[10])
            dense = torch.empty(shape, dtype=torch.int32, device=dev)  # ... allocate exactly ...
            if dense.numel() == 0:
                break
            head = call(dense)                                         # ... emit
            if (head[12], head[11], head[10]) == shape:
                break                                                  # else a new window came in between: allocate again
        return head, dense

    while True:
        head, dense = run(1 if invert and not signed else 0)
        far = head[15]
        if signed:
            other_head, other = run(1)
            if other_head[4:13] != head[4:13]:
                continue                                               # the window moved between the two: both again
            dense = signed_squared(dense, other)
            far += other_head[15]
        break
    n = (head[12], head[11], head[10])
    at = head[14]
    deepest = (head[9] + at // (n[1] * n[2]), head[8] + at // n[2] % n[1], head[7] + at % n[2]) if dense.numel() else (head[9], head[8], head[7])
    return DistanceField(squared=dense, begin=(head[9], head[8], head[7]), offset=(head[6], head[5], head[4]), inside_voxels=head[1],
                         targets=head[0], far_voxels=far, max_squared=head[3], deepest=deepest, lod=lod, background=head[13],
                         scale_factor=scale, volume=volume)
