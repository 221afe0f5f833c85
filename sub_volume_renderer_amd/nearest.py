"""The nearest source of every voxel of what a LOD holds in HBM (the exact feature transform): ``SubVolume.nearest`` over
``svr_nearest`` (include/svr.h), which gives ``svr_distance``'s squared distances without a border and, beside them, the
dense index of the source that attains each and the label there; :class:`NearestField`, which carries the three dense
volumes; and ``SubVolume.expand_labels``, the objects grown by r voxels without merging them."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._box_pass import box_pass, level32
from ._wobject import label_ids, lod_center_to_world
from .distance import FAR, DistanceField, _square

__all__ = ["NearestField", "nearest", "nearest_arguments", "expand_labels"]


@dataclass
class NearestField(DistanceField):
    """The result of one ``SubVolume.nearest`` call: a :class:`DistanceField` made without a border, and for every voxel
    the source nearest to it.  Among the sources at the smallest distance the first in (z, y, x) order is taken.  A voxel
    that is no target is its own nearest source."""

    index: "object" = None    # torch i32 [n_z, n_y, n_x]: (z n_y + y) n_x + x of the nearest source in the box, -1 at a FAR target
    label: "object" = None    # torch u32 of that shape: the label at that voxel, 0 at a FAR target; None with with_labels=False

    def nearest_voxel(self):
        """The nearest source of every voxel as i32 [n_z, n_y, n_x, 3]: absolute LOD voxels (z, y, x), -1 thrice at a
        ``FAR`` target.  On the device."""
        import torch

        nz, ny, nx = (int(v) for v in self.index.shape)
        i = self.index
        rel = torch.stack([torch.div(i, ny * nx, rounding_mode="floor"), torch.div(i, nx, rounding_mode="floor") % ny, i % nx], dim=-1)
        begin = torch.tensor([int(v) for v in self.begin], dtype=torch.int32, device=i.device)
        return torch.where((i < 0).unsqueeze(-1), torch.full_like(rel, -1), rel + begin).to(torch.int32)

    def vector(self):
        """The displacement (z, y, x) from every voxel to its nearest source as i32 [n_z, n_y, n_x, 3]: its squared length
        is ``squared``; 0 at a source and at a ``FAR`` target.  The thickness direction at a voxel."""
        import torch

        shape = tuple(int(v) for v in self.index.shape)
        own = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.int32, device=self.index.device) for n in shape], indexing="ij"), dim=-1)
        begin = torch.tensor([int(v) for v in self.begin], dtype=torch.int32, device=self.index.device)
        there = self.nearest_voxel()
        return torch.where((self.index < 0).unsqueeze(-1), torch.zeros_like(there), there - (own + begin))

    def expanded(self, r):
        """``label`` where the voxel lies at most ``r`` voxels from its nearest source, 0 elsewhere, as u32 on the device.
        A source has the distance 0 and keeps its own label; a ``FAR`` target is never in it.  On a field made with
        ``invert=True`` over the segmentation: the objects grown by ``r`` voxels, every grown voxel taking the label of
        the nearest object (``skimage.segmentation.expand_labels``)."""
        import torch

        limit = _square(r)
        if self.label is None:
            raise ValueError("nearest: expanded() needs the labels; the field was made with with_labels=False")
        bits = self.label.view(torch.int32)                            # the same 32 bits: torch selects on signed integers
        return torch.where(self.squared <= limit, bits, torch.zeros_like(bits)).view(torch.uint32)

    def nearest_position(self, position):
        """The world-space position (x, y, z) of the centre of the nearest source of the voxel that holds the world-space
        ``position``, for :meth:`SubVolume.center_on_position`: a picked point snapped to the surface.  None where the
        point lies outside the box or its voxel has no source."""
        voxel = self._voxel(position)
        if voxel is None:
            return None
        i = int(self.index[voxel])
        if i < 0:
            return None
        nz, ny, nx = (int(v) for v in self.index.shape)
        there = np.array([i // (ny * nx), i // nx % ny, i % nx], np.float64) + np.asarray(self.begin, np.float64)
        return lod_center_to_world(self.volume, there, self.scale_factor)


def nearest_arguments(level, labels, background, invert, with_labels):
    """What ``SubVolume.nearest`` checks before it touches the device -> ``(mode, ids, level, ignore_zero, invert,
    with_labels)``: ``level`` (a number that is not NaN in float32) and ``labels`` exclude one another, the switches are
    bools; anything else is a ``ValueError``."""
    for name, v in (("background", background), ("invert", invert), ("with_labels", with_labels)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"nearest: {name} must be True or False")
    if level is not None and labels is not None:
        raise ValueError("nearest: give level= or labels=, not both")
    if level is None:
        ids = label_ids(labels) if labels is not None else None
        return (N.COMPONENTS_LABELS, ids, 0.0, 0 if background else 1, 1 if invert else 0, bool(with_labels))
    return (N.COMPONENTS_LEVEL, None, level32("nearest", level), 0, 1 if invert else 0, bool(with_labels))


def nearest(volume, level=None, labels=None, background=False, invert=False, with_labels=True, lod: int = 0, box=None, stream=None) -> NearestField:
    """``SubVolume.nearest``: see there."""
    import torch

    p = N.NearestParams()
    p.mode, ids, p.level, p.ignore_zero, p.invert, with_labels = nearest_arguments(level, labels, background, invert, with_labels)
    lod, scale, dev, c_call = box_pass(volume, "svr_nearest", p, lod, box, ids, stream)

    def call(d2, index, label):
        ptr = lambda t: None if t is None else t.data_ptr()
        return c_call(16, lambda header: N.NearestOutputs(ptr(d2), ptr(index), ptr(label), 0 if d2 is None else d2.numel(), header), d2, index, label)

    head = call(None, None, None)                                      # count ...
    while True:
        shape = (head[12], head[11], head[10])
        d2 = torch.empty(shape, dtype=torch.int32, device=dev)         # ... allocate exactly ...
        index = torch.empty(shape, dtype=torch.int32, device=dev)
        label = torch.empty(shape, dtype=torch.uint32, device=dev) if with_labels else None
        if d2.numel() == 0:
            break
        head = call(d2, index, label)                                  # ... emit
        if (head[12], head[11], head[10]) == shape:
            break                                                      # else a new window came in between: allocate again
    n = (head[12], head[11], head[10])
    at = head[14]
    deepest = (head[9] + at // (n[1] * n[2]), head[8] + at // n[2] % n[1], head[7] + at % n[2]) if d2.numel() else (head[9], head[8], head[7])
    return NearestField(squared=d2, begin=(head[9], head[8], head[7]), offset=(head[6], head[5], head[4]), inside_voxels=head[1],
                        targets=head[0], far_voxels=head[15], max_squared=head[3], deepest=deepest, lod=lod, background=head[13],
                        scale_factor=scale, volume=volume, index=index, label=label)


def expand_labels(volume, r, labels=None, lod: int = 0, box=None):
    """``SubVolume.expand_labels``: see there."""
    _square(r)                                                         # a bad r before the device is touched
    return nearest(volume, labels=labels, invert=True, lod=lod, box=box).expanded(r)
