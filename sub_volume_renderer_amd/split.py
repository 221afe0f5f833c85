"""Touching objects split on the device: ``SubVolume.split`` over ``svr_split`` (include/svr.h), the watershed of the
squared distances of ``SubVolume.distance``: every inside voxel climbs to the deepest point it can reach, and two such
basins stay one region where the lower of their peaks stands less than ``merge`` voxels above the pass between them.
:class:`SplitLabels` carries the dense volume of region numbers and one row per region."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._wobject import finest_box, lod_center_to_world
from .components import ComponentLabels
from .distance import DistanceField, _square

__all__ = ["SplitLabels", "split", "split_arguments"]


@dataclass
class SplitLabels:
    """The result of one ``SubVolume.split`` call.  Regions are numbered 1 .. ``count`` in the order of their seeds (the
    first of their summits in z, then y, then x); row ``id - 1`` of every per-region tensor belongs to region ``id``.
    Coordinates are LOD voxels in numpy order (z, y, x)."""

    ids: "object"             # torch i32 [n_z, n_y, n_x]   0 outside, else the region number; voxel [0, 0, 0] is ``begin``
    count: int
    basins: int               # summits of the ascent in all: the regions before any were merged
    begin: tuple              # the first voxel of the box (the distance field's)
    offset: tuple             # the window offset of the LOD
    inside_voxels: int
    voxels: "object"          # torch i64 [count]
    region_basins: "object"   # torch i64 [count]      summits that were merged into the region
    peak_squared: "object"    # torch i64 [count]      the squared distance at ``top``
    top: "object"             # torch i64 [count, 3]   the region's deepest voxel
    lo: "object"              # torch i64 [count, 3]   smallest voxel coordinate
    end: "object"             # torch i64 [count, 3]   largest voxel coordinate + 1
    centroid: "object"        # torch f64 [count, 3]
    lod: int
    merge_squared: int = 1
    connectivity: int = 26
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform
    _host: "dict | None" = None

    def __len__(self):
        return int(self.count)

    def _rows(self):
        if self._host is None:
            self._host = {k: getattr(self, k).cpu().numpy() for k in ("voxels", "peak_squared", "top", "lo", "end")}
        return self._host

    _row = ComponentLabels._row

    def box(self, id):
        """``(begin, end)`` of the region's bounding box in voxels of the finest scale (numpy order, ints), ready for
        :meth:`SubVolume.crop_planes` and ``histogram(box=)``."""
        i, rows = self._row(id), self._rows()
        return finest_box(rows["lo"][i], rows["end"][i], self.scale_factor)

    def position(self, id):
        """The world-space position (x, y, z) of the region's ``top``, its deepest voxel, for
        :meth:`SubVolume.center_on_position`."""
        return lod_center_to_world(self.volume, self._rows()["top"][self._row(id)], self.scale_factor)

    def radius(self, id) -> float:
        """The distance at ``top`` in LOD voxels: the radius of the largest ball inside the region's object; infinity
        where the field is ``FAR``."""
        peak = int(self._rows()["peak_squared"][self._row(id)])
        return float("inf") if peak == N.DISTANCE_FAR else float(np.sqrt(float(peak)))

    # what a region shares with a component: the same rows, the same dense volume
    largest = ComponentLabels.largest
    id_at = ComponentLabels.id_at
    mask = ComponentLabels.mask


def split_arguments(level, labels, merge, connectivity, distance):
    """What ``SubVolume.split`` checks before it touches the device -> ``(merge_squared, connectivity)``: connectivity
    is 6 or 26, ``merge`` a number >= 0 whose square is at most 2^29, and a field the caller holds (``distance=``)
    excludes ``level`` and ``labels``, which made it; anything else is a ``ValueError``."""
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (6, 26):
        raise ValueError("split: connectivity must be 6 or 26")
    try:
        merge_squared = _square(merge)
    except ValueError:
        raise ValueError("split: merge must be a number >= 0") from None
    if merge_squared > N.SPLIT_MAX_MERGE:
        raise ValueError("split: merge * merge must be at most 2^29")
    if distance is not None:
        if not isinstance(distance, DistanceField):
            raise ValueError("split: distance must be a DistanceField")
        if level is not None or labels is not None:
            raise ValueError("split: a DistanceField was made from its own level= or labels=; give distance= alone")
    return merge_squared, int(connectivity)


def split(volume, level=None, labels=None, background=False, merge=1.0, connectivity=26, border=True, lod: int = 0, box=None,
          distance=None, stream=None) -> SplitLabels:
    """``SubVolume.split``: see there."""
    import torch

    sp = N.SplitParams()
    sp.merge_squared, sp.connectivity = split_arguments(level, labels, merge, connectivity, distance)
    field = distance if distance is not None else volume.distance(level=level, labels=labels, background=background, border=border,
                                                                   lod=lod, box=box, stream=stream)
    squared = field.squared
    if squared.dtype != torch.int32 or squared.dim() != 3 or not squared.is_cuda:
        raise ValueError("split: distance.squared must be an int32 [z, y, x] tensor on the device")
    squared = squared.contiguous()
    dev = squared.device
    shape = tuple(int(v) for v in squared.shape)

    def result(ids, count, basins, inside, records):
        r64 = records.view(torch.int64) if count else torch.empty((0, N.SPLIT_RECORD_BYTES // 8), dtype=torch.int64, device=dev)
        begin = torch.tensor(tuple(field.begin), dtype=torch.int64, device=dev)
        voxels = r64[:, 1].contiguous()
        centroid = begin.to(torch.float64) + (r64[:, 2:5].to(torch.float64) / voxels.to(torch.float64).unsqueeze(1)).flip(1)
        return SplitLabels(ids=ids, count=count, basins=basins, begin=tuple(field.begin), offset=tuple(field.offset), inside_voxels=inside,
                           voxels=voxels, region_basins=records[:, 1].to(torch.int64), peak_squared=records[:, 19].to(torch.int64),
                           top=begin + records[:, 10:13].flip(1).to(torch.int64), lo=begin + records[:, 13:16].flip(1).to(torch.int64),
                           end=begin + records[:, 16:19].flip(1).to(torch.int64) + 1, centroid=centroid, lod=field.lod,
                           merge_squared=int(sp.merge_squared), connectivity=int(sp.connectivity), scale_factor=tuple(field.scale_factor),
                           volume=field.volume if field.volume is not None else volume)

    empty_records = torch.empty((0, N.SPLIT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
    if squared.numel() == 0:                                           # an empty window: nothing to call
        return result(torch.empty(shape, dtype=torch.int32, device=dev), 0, 0, 0, empty_records)

    handle = volume.prepare()
    side = torch.cuda.ExternalStream(int(stream), device=dev) if stream is not None else None
    raw_stream = volume._plane_stream(stream)
    sp.height = squared.data_ptr()
    sp.n[:] = shape[::-1]

    def call(ids, records):
        header = torch.empty(16, dtype=torch.int64, device=dev)
        if side is not None:
            torch.cuda.current_stream(dev).synchronize()               # the field and the allocator's memory may still be in use there
        out = N.SplitOutputs(None if ids is None else ids.data_ptr(), 0 if ids is None else ids.numel(),
                             None if records is None else records.data_ptr(), 0 if records is None else records.shape[0], header.data_ptr())
        N.check(N.lib().svr_split(handle, C.byref(sp), C.byref(out), C.c_void_p(raw_stream)), "svr_split")
        if side is not None:
            for t in (ids, records, header, squared):
                if t is not None:
                    t.record_stream(side)
            side.synchronize()
        return [int(v) for v in header.cpu().numpy()]                  # synchronises

    head = call(None, None)                                            # count ...
    count = head[0]
    ids = torch.empty(shape, dtype=torch.int32, device=dev)            # ... allocate exactly ...
    records = torch.empty((count, N.SPLIT_RECORD_BYTES // 4), dtype=torch.int32, device=dev) if count else empty_records
    head = call(ids, records if count else None)                       # ... emit: the field is the caller's and has not changed
    return result(ids, count, head[4], head[1], records)
