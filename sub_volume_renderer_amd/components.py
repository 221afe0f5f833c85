"""Connected components of what a LOD holds in HBM: ``SubVolume.components`` over ``svr_components`` (include/svr.h),
which labels the blobs of a level set (``level``) or the pieces of the segmentation's objects on the device, and
:class:`ComponentLabels`, which carries the dense volume of component numbers and one row per component."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._box_pass import box_pass, level32
from ._wobject import finest_box, label_ids, lod_center_to_world

__all__ = ["ComponentLabels", "components", "components_arguments"]


@dataclass
class ComponentLabels:
    """The result of one ``SubVolume.components`` call.  Components are numbered 1 .. ``count`` in the order of their
    first voxels (z, then y, then x), the numbering of ``scipy.ndimage.label``; row ``id - 1`` of every per-component
    tensor belongs to component ``id``.  Coordinates are LOD voxels in numpy order (z, y, x)."""

    ids: "object"             # torch i32 [n_z, n_y, n_x]   0 outside, else the component number; voxel [0, 0, 0] is ``begin``
    count: int
    begin: tuple              # the first voxel of the labelled box (box and window intersected)
    offset: tuple             # the window offset of the LOD
    inside_voxels: int
    background: int           # label-0 voxels left out by background=False
    label: "object"           # torch i64 [count]      the label of the component's first voxel (0 with level=)
    voxels: "object"          # torch i64 [count]
    first: "object"           # torch i64 [count, 3]   the first voxel
    lo: "object"              # torch i64 [count, 3]   smallest voxel coordinate
    end: "object"             # torch i64 [count, 3]   largest voxel coordinate + 1
    centroid: "object"        # torch f64 [count, 3]   window offset + sum / voxels
    lod: int
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform
    _host: "dict | None" = None

    def __len__(self):
        return int(self.count)

    def _rows(self):
        if self._host is None:
            self._host = {k: getattr(self, k).cpu().numpy() for k in ("label", "voxels", "lo", "end", "centroid")}
        return self._host

    def _row(self, id) -> int:
        if isinstance(id, (bool, np.bool_)) or not isinstance(id, (int, np.integer)) or not 1 <= id <= self.count:
            raise KeyError(id)
        return int(id) - 1

    def box(self, id):
        """``(begin, end)`` of the component's bounding box in voxels of the finest scale (numpy order, ints), ready for
        :meth:`SubVolume.crop_planes` and ``histogram(box=)``: :func:`finest_box` of its LOD box."""
        i, rows = self._row(id), self._rows()
        return finest_box(rows["lo"][i], rows["end"][i], self.scale_factor)

    def position(self, id):
        """The world-space position (x, y, z) of the component's centroid, for :meth:`SubVolume.center_on_position`:
        what ``ObjectTable.position`` computes for an object."""
        return lod_center_to_world(self.volume, self._rows()["centroid"][self._row(id)], self.scale_factor)

    def largest(self, k: int = 1):
        """The numbers of the ``k`` largest components, by descending voxel count, ties by ascending number."""
        voxels = self._rows()["voxels"]
        order = np.lexsort((np.arange(len(voxels)), -voxels.astype(np.int64)))
        return [int(i) + 1 for i in order[:max(int(k), 0)]]

    def id_at(self, position) -> int:
        """The number of the component that holds the world-space ``position`` (x, y, z), 0 when the voxel there is
        outside every component or outside the labelled box: the component under a picked point."""
        world = np.array([float(v) for v in position] + [1.0], np.float64)
        data = (np.linalg.inv(np.asarray(self.volume.world.matrix, np.float64)) @ world)[:3][::-1]          # numpy order
        # the LOD voxel that holds finest data coordinate d: the inverse of lod_center_to_data, rounded to the voxel
        voxel = np.floor((data + 0.5) * np.asarray(self.scale_factor, np.float64)).astype(np.int64) - np.asarray(self.begin, np.int64)
        if np.any(voxel < 0) or np.any(voxel >= np.asarray(tuple(self.ids.shape), np.int64)):
            return 0
        return int(self.ids[int(voxel[0]), int(voxel[1]), int(voxel[2])])

    def pieces(self, label):
        """The numbers of the components whose ``label`` is this one: the pieces of a segmentation object."""
        return [int(i) + 1 for i in np.nonzero(self._rows()["label"] == int(label))[0]]

    def mask(self, ids):
        """The voxels of these components as a bool tensor of ``ids``' shape, on the device."""
        import torch

        want = torch.tensor([int(i) for i in ([ids] if isinstance(ids, (int, np.integer)) else ids)], dtype=torch.int32, device=self.ids.device)
        return torch.isin(self.ids, want) & (self.ids != 0)


def components_arguments(level, labels, background, join, connectivity):
    """What ``SubVolume.components`` checks before it touches the device -> ``(mode, ids, level, ignore_zero, join,
    connectivity)``: ``level`` (a number that is not NaN in float32) and ``labels`` exclude one another, connectivity is
    6 or 26; anything else is a ``ValueError``."""
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (6, 26):
        raise ValueError("components: connectivity must be 6 or 26")
    if level is not None and labels is not None:
        raise ValueError("components: give level= or labels=, not both")
    if level is None:
        ids = label_ids(labels) if labels is not None else None
        return N.COMPONENTS_LABELS, ids, 0.0, 0 if background else 1, 1 if join else 0, int(connectivity)
    return N.COMPONENTS_LEVEL, None, level32("components", level), 0, 0, int(connectivity)


def components(volume, level=None, labels=None, background=False, join=False, connectivity=6, lod: int = 0, box=None,
               stream=None) -> ComponentLabels:
    """``SubVolume.components``: see there."""
    import torch

    cp = N.ComponentsParams()
    cp.mode, ids, cp.level, cp.ignore_zero, cp.join_labels, cp.connectivity = components_arguments(level, labels, background, join, connectivity)
    lod, scale, dev, c_call = box_pass(volume, "svr_components", cp, lod, box, ids, stream)

    def call(dense, records):
        co = lambda header: N.ComponentsOutputs(None if dense is None else dense.data_ptr(), 0 if dense is None else dense.numel(),
                                                None if records is None else records.data_ptr(), 0 if records is None else records.shape[0], header)
        return c_call(16, co, dense, records)

    head = call(None, None)                                            # count ...
    while True:
        count, shape = head[0], (head[12], head[11], head[10])
        dense = torch.empty(shape, dtype=torch.int32, device=dev)      # ... allocate exactly ...
        records = torch.empty((count, N.COMPONENT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
        if dense.numel() == 0:
            break
        head = call(dense, records if count else None)                 # ... emit
        if (head[0], (head[12], head[11], head[10])) == (count, shape):
            break                                                      # else an upload or a new window came in between: allocate again
    # record fields by their 4- and 8-byte columns (svr_component_record)
    r64 = records.view(torch.int64) if count else torch.empty((0, N.COMPONENT_RECORD_BYTES // 8), dtype=torch.int64, device=dev)
    voxels = r64[:, 1].contiguous()
    offset = torch.tensor([head[4], head[5], head[6]], dtype=torch.float64, device=dev)
    centroid = (offset + r64[:, 2:5].to(torch.float64) / voxels.to(torch.float64).unsqueeze(1)).flip(1)
    return ComponentLabels(ids=dense, count=count, begin=(head[9], head[8], head[7]), offset=(head[6], head[5], head[4]),
                           inside_voxels=head[1], background=head[13], label=records[:, 1].to(torch.int64) & 0xFFFFFFFF, voxels=voxels,
                           first=records[:, 10:13].flip(1).to(torch.int64), lo=records[:, 13:16].flip(1).to(torch.int64),
                           end=records[:, 16:19].flip(1).to(torch.int64) + 1, centroid=centroid, lod=lod, scale_factor=scale, volume=volume)
