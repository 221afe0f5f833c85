"""Display-side segmentation outlines and selected-object highlighting (``svr_outline``, include/svr.h).

The reference colours each hit pixel by its label's hue from a short table, so touching objects of one hue merge;
its FUTURE.md ("Tracing Objects") asks for a second pass that finds label edges in the rendered label image and
draws them over the intensity image.  This is that pass: one HIP kernel over the planes a render already wrote.
The outlined RGBA feeds :func:`compose` like the render's own::

    compose(volume, dataclasses.replace(result, rgba=outline(volume, result)))
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def _palette(volume, device):
    """The material's HSV table as a device tensor [n, 4], rebuilt when the material changed."""
    import torch

    m = volume.material
    cached = volume.__dict__.get("_outline_palette")
    if cached is not None and cached[0] is m and cached[1] == m._version and cached[2].device == device:
        return cached[2]
    table = torch.from_numpy(np.ascontiguousarray(m._u["colors"], np.float32)).to(device)
    volume.__dict__["_outline_palette"] = (m, m._version, table)
    return table


def _selection(selected, device):
    """Any iterable of ints or an integer tensor -> unique ids as u32 bit patterns in an int32 tensor, ascending as
    u32.  int32 tensors are read as bit patterns (like ``RenderResult.label``); other values must lie in [0, 2^32)."""
    import torch

    if isinstance(selected, torch.Tensor):
        if selected.dtype.is_floating_point or selected.dtype.is_complex or selected.dtype == torch.bool:
            raise TypeError("selected must hold integers")
        ids = selected.reshape(-1).to(device=device, dtype=torch.int64)
        if selected.dtype == torch.int32:
            ids = ids & 0xFFFFFFFF
    else:
        vals = list(selected)
        if any(not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) for v in vals):
            raise TypeError("selected must hold integers")
        ids = torch.tensor([int(v) for v in vals], dtype=torch.int64, device=device)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) > 0xFFFFFFFF):
        raise ValueError("selected ids must lie in [0, 2^32)")
    ids = torch.unique(ids, sorted=True)
    return torch.where(ids >= 2**31, ids - 2**32, ids).to(torch.int32).contiguous()


def outline(volume, result, *, width: int = 1, color=(0.0, 0.0, 0.0, 1.0), color_by_label: bool = False,
            depth_tolerance=None, selected=None, dim_unselected: float = 1.0, only_selected: bool = False, out=None,
            edge_mask=None):
    """Draw label edges of one render over its RGBA (definition: ``svr_outline`` in include/svr.h).

    ``result``: a :class:`RenderResult` of ``volume.render`` (its rgba, label and flags planes; depth when
    ``depth_tolerance`` is given).  A frame gathered by ``distributed.TiledFrame`` is passed as
    ``RenderResult(rgba, depth, label, flags, None)`` of its planes.  A tile rendered with ``region=`` is an image of
    its own here: pixels outside it are not neighbours, so outline a tiled frame after the gather.

    ``width``: window radius r in pixels, 1 .. 16.  ``color``: outline RGBA in linear light (alpha = opacity); with
    ``color_by_label`` the rgb is the label's hue from ``volume.material.colors`` at full value.
    ``depth_tolerance``: also outline where a neighbour of the same label lies more than this far away in the depth
    plane.  ``selected``: label ids (iterable of ints or an integer tensor); pixels of other labels are dimmed by
    ``dim_unselected``, and with ``only_selected`` only selected objects are outlined.  ``out``: contiguous float32
    tensor [h, w, 4], may be ``result.rgba`` itself.  ``edge_mask``: optional contiguous uint8 tensor [h, w] that
    receives 1 on edge pixels.  Enqueued on the current torch stream; returns ``out``."""
    import torch

    rgba = result.rgba
    if rgba.dim() != 3 or rgba.shape[2] != 4 or rgba.dtype != torch.float32 or not rgba.is_contiguous() or not rgba.is_cuda:
        raise ValueError("result.rgba must be a contiguous float32 CUDA tensor [h, w, 4]")
    h, w = rgba.shape[:2]
    dev = rgba.device

    def plane(t, name, dtype):
        if t is None:
            raise ValueError(f"outline needs the render's {name} plane")
        if tuple(t.shape) != (h, w) or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"result.{name} must be a contiguous {dtype} tensor [h, w] on {dev}")
        return t

    label = plane(result.label, "label", torch.int32)
    flags = plane(result.flags, "flags", torch.uint8)
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= int(width) <= 16:
        raise ValueError("width must be an integer in [1, 16]")
    color = tuple(float(v) for v in color)
    if len(color) != 4:
        raise ValueError("color must be RGBA")
    if not 0.0 <= color[3] <= 1.0:
        raise ValueError("the outline opacity color[3] must be in [0, 1]")
    if not 0.0 <= float(dim_unselected) <= 1.0:
        raise ValueError("dim_unselected must be in [0, 1]")
    depth = None
    if depth_tolerance is not None:
        depth_tolerance = float(depth_tolerance)
        if not depth_tolerance >= 0.0:
            raise ValueError("depth_tolerance must be >= 0 (None turns the depth test off)")
        depth = plane(result.depth, "depth", torch.float32)
    if out is None:
        out = torch.empty_like(rgba)
    if tuple(out.shape) != (h, w, 4) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 tensor [h, w, 4] on the render's device")
    if edge_mask is not None and (tuple(edge_mask.shape) != (h, w) or edge_mask.dtype != torch.uint8
                                  or not edge_mask.is_contiguous() or edge_mask.device != dev):
        raise ValueError("edge_mask must be a contiguous uint8 tensor [h, w] on the render's device")
    colors = _palette(volume, dev) if color_by_label else None
    if colors is not None and colors.shape[0] == 0:
        raise ValueError("color_by_label needs at least one material color")
    sel = _selection(selected, dev) if selected is not None else None
    nsel = int(sel.numel()) if sel is not None else 0

    q = N.OutlineParams()
    q.radius = int(width)
    q.depth_tolerance = depth_tolerance if depth_tolerance is not None else -1.0
    q.color_by_label = 1 if color_by_label else 0
    q.color[:] = color
    q.dim_unselected = float(dim_unselected)
    q.only_selected = 1 if only_selected else 0
    if h == 0 or w == 0:
        return out
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    N.check(
        N.lib().svr_outline(
            volume._rings.handle, ptr(rgba), ptr(depth), ptr(label), ptr(flags), w, h, C.byref(q),
            ptr(colors), int(colors.shape[0]) if colors is not None else 0, ptr(sel), nsel, ptr(out), ptr(edge_mask),
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
        "svr_outline")
    return out
