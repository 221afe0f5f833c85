"""Contacts between the objects a LOD holds in HBM: ``SubVolume.contacts`` over ``svr_contacts`` (include/svr.h), which
fills a table of touching label pairs on the device, and :class:`ContactTable`, the region adjacency graph it gives:
one row per unordered pair with its contact area per face normal, where the contact lies, and the values along it."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._box_pass import box_pass
from ._wobject import finest_box, label_ids, lod_center_to_data, objects_capacity

__all__ = ["ContactTable", "contacts", "table_from_records"]


@dataclass
class ContactTable:
    """The occupied records of one ``svr_contacts`` call, compacted and sorted by (a, b) on the device.  A row is the
    contact of objects ``a < b``: the faces between a voxel of the one and a voxel of the other.  Coordinates and the
    columns of ``faces`` are in numpy order (z, y, x), in LOD voxels; a face belongs to the voxel p on its lower side,
    and its centre lies half a voxel beyond p along its normal."""

    a: "object"               # torch i64 [n]        the smaller label, ascending
    b: "object"               # torch i64 [n]        the larger label, ascending within one a
    faces: "object"           # torch i64 [n, 3]     faces whose normal is z, y, x
    area: "object"            # torch i64 [n]        their sum
    begin: "object"           # torch i64 [n, 3]     smallest coordinate of the owning voxels
    end: "object"             # torch i64 [n, 3]     largest coordinate of the owning voxels + 1
    centroid: "object"        # torch f64 [n, 3]     mean face centre: window offset + sum2 / (2 * area)
    finite: "object"          # torch i64 [n]        finite values among the two each face offers
    mean: "object"            # torch f64 [n]        of the finite values; NaN where there are none
    min: "object"             # torch f32 [n]        +inf where finite == 0
    max: "object"             # torch f32 [n]        -inf where finite == 0
    considered: int           # faces that took part
    background: int           # faces with label 0 left out by background=False
    voxels: int               # voxels of the box the faces were looked for in
    lod: int
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform
    _host: "dict | None" = None

    def __len__(self):
        return int(self.a.numel())

    def _rows(self):
        if self._host is None:
            host = {k: getattr(self, k).cpu().numpy() for k in ("a", "b", "faces", "area", "begin", "end", "centroid")}
            host["row"] = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(host["a"], host["b"]))}
            self._host = host
        return self._host

    def index(self, a, b) -> int:
        """The row of the pair, given in either order; ``KeyError`` when the table does not hold it."""
        a, b = int(a), int(b)
        pair = (a, b) if a < b else (b, a)
        try:
            return self._rows()["row"][pair]
        except KeyError:
            raise KeyError(pair) from None

    def neighbours(self, id):
        """``(ids, areas)``, int64 arrays: the objects that ``id`` touches and the contact areas in faces, the largest
        area first, ties by the smaller id."""
        rows = self._rows()
        mine = (rows["a"] == int(id)) | (rows["b"] == int(id))
        partner = np.where(rows["a"] == int(id), rows["b"], rows["a"])[mine].astype(np.int64)
        area = rows["area"][mine].astype(np.int64)
        order = np.lexsort((partner, -area))
        return partner[order], area[order]

    def surface(self, id) -> int:
        """The faces of ``id`` with anything else in the table: its whole surface inside the box when the call had
        ``background=True`` and no ``labels`` that leave a partner out."""
        return int(self.neighbours(id)[1].sum())

    def data_area(self):
        """Per row, the contact area in squared voxels of the finest scale: a face whose normal is axis k covers
        ``prod(1 / scale_j for j != k)`` of them.  float64, on the table's device."""
        import torch

        inv = [1.0 / float(s) for s in self.scale_factor]
        per_face = torch.tensor([inv[1] * inv[2], inv[0] * inv[2], inv[0] * inv[1]], dtype=torch.float64, device=self.faces.device)
        return (self.faces.to(torch.float64) * per_face).sum(dim=1)

    def box(self, a, b):
        """``(begin, end)`` of the box of the contact's owning voxels in voxels of the finest scale (numpy order, ints),
        ready for :meth:`SubVolume.crop_planes` and ``histogram(box=)``: :func:`finest_box` of the row's LOD box.  The
        voxels on the other side of the faces lie at most one LOD voxel beyond ``end``."""
        i, rows = self.index(a, b), self._rows()
        return finest_box(rows["begin"][i], rows["end"][i], self.scale_factor)

    def position(self, a, b):
        """The world-space position (x, y, z) of the contact's mean face centre, for
        :meth:`SubVolume.center_on_position`: ``ObjectTable.position``'s arithmetic on the centroid."""
        data = lod_center_to_data(self._rows()["centroid"][self.index(a, b)], self.scale_factor)[::-1]      # shader order
        world = np.asarray(self.volume.world.matrix, np.float64) @ np.array([*data, 1.0])
        return tuple(float(v) for v in world[:3])


def table_from_records(records, head, float_ring, lod, scale_factor=(1.0, 1.0, 1.0), volume=None) -> ContactTable:
    """The records of one call (an int64 tensor [capacity, 14]: ``svr_contact_record`` by its 8-byte columns, on any
    device) and its 8 header words as ints -> the table, compacted and sorted with torch ops where the records are.
    ``float_ring``: value_sum holds the bits of an f64 sum."""
    import torch

    w32 = records.view(torch.int32)
    rows = torch.nonzero(records[:, 0] != 0).reshape(-1)
    a = w32[rows, 0].to(torch.int64) & 0xFFFFFFFF
    b = w32[rows, 1].to(torch.int64) & 0xFFFFFFFF
    # by (a, b) in two stable passes: one key a << 32 | b as int64 would misorder labels of 2^31 and above
    order = torch.sort(b, stable=True)[1]
    order = order[torch.sort(a[order], stable=True)[1]]
    rows = rows[order]
    r64, r32 = records[rows], w32[rows]
    faces = r64[:, 1:4]
    area = faces.sum(dim=1)
    finite = r64[:, 10]
    offset = torch.tensor([head[4], head[5], head[6]], dtype=torch.float64, device=records.device)
    centroid = (offset + r64[:, 4:7].to(torch.float64) / (2.0 * area.to(torch.float64)).unsqueeze(1)).flip(1)
    total = r64[:, 11].contiguous().view(torch.float64) if float_ring else r64[:, 11].to(torch.float64)
    mean = torch.where(finite > 0, total / finite.to(torch.float64), torch.full_like(total, float("nan")))
    vmm = r32[:, 24:26].contiguous().view(torch.float32)
    return ContactTable(a=a[order], b=b[order], faces=faces.flip(1).contiguous(), area=area, begin=r32[:, 14:17].flip(1).to(torch.int64),
                        end=r32[:, 17:20].flip(1).to(torch.int64) + 1, centroid=centroid, finite=finite.contiguous(), mean=mean,
                        min=vmm[:, 0].contiguous(), max=vmm[:, 1].contiguous(), considered=int(head[1]), background=int(head[3]),
                        voxels=int(head[7]), lod=lod, scale_factor=tuple(float(v) for v in scale_factor), volume=volume)


def contacts(volume, lod: int = 0, box=None, labels=None, background: bool = False, capacity=None, stream=None) -> ContactTable:
    """``SubVolume.contacts``: see there."""
    import torch

    ids = label_ids(labels) if labels is not None else None
    cap, automatic = objects_capacity(capacity)             # an id list bounds no pair count: it starts like no list
    cp = N.ContactsParams()
    cp.ignore_zero = 0 if background else 1
    lod, scale, dev, c_call = box_pass(volume, "svr_contacts", cp, lod, box, ids, stream)
    while True:
        records = torch.empty((cap, N.CONTACT_RECORD_BYTES // 8), dtype=torch.int64, device=dev)
        cp.capacity = cap
        head = c_call(8, lambda header: N.ContactsOutputs(records.data_ptr(), header), records)
        if head[2] == 0:
            break
        if not automatic:
            raise ValueError(f"contacts: capacity {cap} is too small: {head[2]} of {head[1]} faces belong to pairs "
                             f"that found no record (pass a larger capacity, or None)")
        if cap >= N.CONTACTS_MAX_CAPACITY:
            raise ValueError(f"contacts: more than {N.CONTACTS_MAX_CAPACITY} distinct pairs of labels touch")
        cap = min(cap * 8, N.CONTACTS_MAX_CAPACITY)
    return table_from_records(records, head, volume._rings.density_storage == "float32", lod, scale, volume)
