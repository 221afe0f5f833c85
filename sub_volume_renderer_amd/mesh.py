"""Surface meshes of what a LOD holds in HBM: ``SubVolume.mesh`` over ``svr_mesh`` (include/svr.h), which extracts a
picked object (``labels``) or a level set (``level``) on the device as vertices and triangles, and :class:`SurfaceMesh`,
which carries them and measures or exports them."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._box_pass import box_pass, level32
from ._wobject import label_ids

__all__ = ["SurfaceMesh", "mesh", "mesh_arguments"]


@dataclass
class SurfaceMesh:
    """The result of one ``SubVolume.mesh`` call.  ``vertices`` are LOD voxels in shader order (x, y, z) relative to
    ``offset``, integer c being the centre of voxel c; triangles wind so that their normals point out of the object."""

    vertices: "object"        # torch f32 [V, 3]     x, y, z, relative to ``offset``
    triangles: "object"       # torch i32 [T, 3]
    offset: tuple             # the window offset (x, y, z) of the LOD, LOD voxels
    inside_voxels: int        # voxels of the box that are inside the surface
    lod: int
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform

    def __len__(self):
        return int(self.triangles.shape[0])

    def data_vertices(self):
        """The vertices as data coordinates of the finest scale (torch f64 [V, 3], shader order): what
        ``lod_center_to_data`` computes, ``(c + 0.5) / scale - 0.5`` per axis, on the device."""
        import torch

        dev = self.vertices.device
        off = torch.tensor([float(v) for v in self.offset], dtype=torch.float64, device=dev)
        scale = torch.tensor([float(v) for v in self.scale_factor[::-1]], dtype=torch.float64, device=dev)    # shader order
        return (self.vertices.to(torch.float64) + off + 0.5) / scale - 0.5

    def world_vertices(self):
        """The vertices in world space (torch f64 [V, 3]): :meth:`data_vertices` through the volume's world transform
        (the identity for a mesh that carries no volume)."""
        import torch

        data = self.data_vertices()
        if self.volume is None:
            return data
        m = torch.tensor(np.asarray(self.volume.world.matrix, np.float64), dtype=torch.float64, device=data.device)
        return data @ m[:3, :3].T + m[:3, 3]

    def _corners(self):
        w = self.world_vertices()
        t = self.triangles.to(w.device).long()
        return w[t[:, 0]], w[t[:, 1]], w[t[:, 2]]

    def area(self) -> float:
        """The surface area in world units: the sum of half the cross products' lengths, in f64 on the device."""
        import torch

        a, b, c = self._corners()
        return float(0.5 * torch.linalg.norm(torch.linalg.cross(b - a, c - a), dim=1).sum())

    def enclosed_volume(self) -> float:
        """The volume the surface encloses in world units, by the divergence sum sum(v0 . (v1 x v2)) / 6 in f64 on the
        device; positive, since the normals point out of the object (a world transform that mirrors flips the sign)."""
        import torch

        a, b, c = self._corners()
        return float((a * torch.linalg.cross(b, c)).sum() / 6.0)

    def write_obj(self, path, world: bool = True):
        """A Wavefront OBJ file of the mesh: ``v x y z`` per vertex (world space, or data coordinates of the finest
        scale with ``world=False``; ``repr`` of the f64 values, so that reading them back gives the same numbers) and
        ``f i j k`` per triangle with 1-based indices."""
        v = (self.world_vertices() if world else self.data_vertices()).cpu().numpy()
        t = self.triangles.cpu().numpy().astype(np.int64) + 1
        with open(path, "w") as f:
            f.write(f"# {len(v)} vertices, {len(t)} triangles, LOD {self.lod}\n")
            f.writelines(f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for p in v)
            f.writelines(f"f {int(q[0])} {int(q[1])} {int(q[2])}\n" for q in t)


def mesh_arguments(labels, level):
    """What ``SubVolume.mesh`` checks before it touches the device -> ``(mode, ids, level)``: exactly one of ``labels``
    (through ``label_ids``) and ``level`` (a number that is not NaN in float32); anything else is a ``ValueError``."""
    if (labels is None) == (level is None):
        raise ValueError("mesh: give exactly one of labels= and level=")
    if labels is not None:
        return N.MESH_LABELS, label_ids(labels), 0.0
    return N.MESH_LEVEL, None, level32("mesh", level)


def mesh(volume, labels=None, level=None, lod: int = 0, box=None, stream=None) -> SurfaceMesh:
    """``SubVolume.mesh``: see there."""
    import torch

    mp = N.MeshParams()
    mp.mode, ids, mp.level = mesh_arguments(labels, level)
    lod, scale, dev, c_call = box_pass(volume, "svr_mesh", mp, lod, box, ids, stream)

    def call(vertices, triangles):
        mo = lambda header: N.MeshOutputs(None if vertices is None else vertices.data_ptr(), None if triangles is None else triangles.data_ptr(),
                                          header, 0 if vertices is None else vertices.shape[0], 0 if triangles is None else triangles.shape[0])
        return c_call(8, mo, vertices, triangles)

    head = call(None, None)                                            # count ...
    while True:
        nv, nt = head[0], head[1]
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)   # ... allocate exactly ...
        triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        if not (nv and nt):
            break
        head = call(vertices, triangles)                               # ... emit
        if (head[0], head[1]) == (nv, nt):
            break                                                      # else an upload landed in between: allocate for the new counts
    return SurfaceMesh(vertices=vertices, triangles=triangles, offset=(head[4], head[5], head[6]), inside_voxels=head[7], lod=lod,
                       scale_factor=scale, volume=volume)
