"""``TransferFunction`` — the colour and opacity table of the composite render mode (``svr_composite``, include/svr.h).

A table of K RGBA entries (2 <= K <= 4096) over the contrast-limited value: entry 0 at ``clim[0]``, entry K-1 at
``clim[1]``, linear interpolation between neighbours on the device.  RGB is kept in linear light; alpha is the opacity
of one voxel's length of material.  :meth:`TransferFunction.device_table` bakes the opacity correction for the march's
sample spacing into the table on the host, so the kernel does plain multiplies and adds per sample.
"""

from __future__ import annotations

import numbers

import numpy as np

MAX_ENTRIES = 4096          # SVR_TF_MAX_ENTRIES


def _srgb_to_linear(c: np.ndarray) -> np.ndarray:
    """The sRGB EOTF in float64."""
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def nominal_step(volume_dimensions) -> np.float32:
    """The march's sample spacing in voxels, as ``svr_render.hip`` computes it in f32 (fs_main.wgsl:20):
    ``min(max(sqrt(max(size)) / 20, 0.1), 0.8)``."""
    mx = max(np.float32(v) for v in volume_dimensions)
    return np.float32(min(max(np.sqrt(np.float32(mx)) / np.float32(20.0), np.float32(0.1)), np.float32(0.8)))


def _rgba(value, what):
    if isinstance(value, (str, bytes)):
        raise ValueError(f"{what} must be four numbers (r, g, b, a)")
    try:
        vals = [float(c) for c in value]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be four numbers (r, g, b, a)") from None
    if len(vals) != 4:
        raise ValueError(f"{what} must be four numbers (r, g, b, a)")
    return vals


class TransferFunction:
    """An immutable RGBA table for ``SubVolumeMaterial(render_mode="composite")``.

    ``table``: K x 4 numbers in [0, 1], 2 <= K <= 4096.  ``srgb=True``: the RGB columns are sRGB-encoded and are
    converted to linear light here (alpha is left as it is)."""

    def __init__(self, table, srgb: bool = False):
        try:
            t = np.array(table, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("the table must be a K x 4 array of numbers") from None
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError(f"the table must have shape (K, 4), not {t.shape}")
        if not 2 <= t.shape[0] <= MAX_ENTRIES:
            raise ValueError(f"the table must have 2 .. {MAX_ENTRIES} entries, not {t.shape[0]}")
        if not np.all(np.isfinite(t)) or t.min() < 0.0 or t.max() > 1.0:
            raise ValueError("every table entry must be finite and in [0, 1]")
        if srgb:
            t[:, :3] = _srgb_to_linear(t[:, :3])
        t.setflags(write=False)
        self._table = t

    @property
    def table(self) -> np.ndarray:
        """The K x 4 float64 table (RGB in linear light, alpha per voxel), read-only."""
        return self._table

    @property
    def size(self) -> int:
        return int(self._table.shape[0])

    def __repr__(self) -> str:
        return f"TransferFunction(size={self.size})"

    @classmethod
    def linear(cls, color=(1.0, 1.0, 1.0), opacity: float = 0.05, size: int = 256) -> "TransferFunction":
        """One colour, alpha rising linearly from 0 at ``clim[0]`` to ``opacity`` at ``clim[1]``."""
        size = cls._check_size(size)
        if isinstance(color, (str, bytes)) or len(color) != 3 or not all(isinstance(c, numbers.Real) for c in color):
            raise ValueError("color must be three numbers (r, g, b)")
        if not isinstance(opacity, numbers.Real):
            raise ValueError("opacity must be a number")
        ramp = np.linspace(0.0, 1.0, size)
        table = np.empty((size, 4), np.float64)
        table[:, :3] = [float(c) for c in color]
        table[:, 3] = float(opacity) * ramp
        return cls(table)

    @classmethod
    def from_points(cls, points, size: int = 256, srgb: bool = False) -> "TransferFunction":
        """Piecewise-linear through ``[(position, (r, g, b, a)), ...]``, positions in [0, 1] in non-decreasing order
        (normalised value: 0 at ``clim[0]``, 1 at ``clim[1]``); constant beyond the first and last point.  Sampled at
        ``size`` evenly spaced positions in float64."""
        size = cls._check_size(size)
        if isinstance(points, (str, bytes)):
            raise ValueError("points must be a list of (position, (r, g, b, a))")
        pos, cols = [], []
        for p in points:
            try:
                x, rgba = p
                x = float(x)
            except (TypeError, ValueError):
                raise ValueError("points must be a list of (position, (r, g, b, a))") from None
            if not 0.0 <= x <= 1.0:
                raise ValueError(f"point positions must be in [0, 1], not {x!r}")
            pos.append(x)
            cols.append(_rgba(rgba, "a point's colour"))
        if not pos:
            raise ValueError("at least one point is required")
        if any(b < a for a, b in zip(pos, pos[1:])):
            raise ValueError("point positions must be in non-decreasing order")
        xs = np.linspace(0.0, 1.0, size)
        cols = np.array(cols, np.float64)
        table = np.stack([np.interp(xs, pos, cols[:, k]) for k in range(4)], axis=1)
        return cls(table, srgb=srgb)

    @staticmethod
    def _check_size(size):
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 2 <= size <= MAX_ENTRIES:
            raise ValueError(f"size must be an integer in 2 .. {MAX_ENTRIES}")
        return int(size)

    def device_table(self, volume_dimensions) -> np.ndarray:
        """The f32 K x 4 table ``svr_set_transfer_function`` receives for a volume of these dimensions: RGB as it
        is, alpha corrected for the march's nominal sample spacing ``rel_step`` (voxels):
        ``a' = 1 - (1 - a) ** rel_step`` in float64, then rounded to f32."""
        rel = float(nominal_step(volume_dimensions))
        out = np.empty(self._table.shape, np.float32)
        out[:, :3] = self._table[:, :3]
        out[:, 3] = 1.0 - (1.0 - self._table[:, 3]) ** rel
        return out


_DEFAULT = None


def default_transfer_function() -> TransferFunction:
    """``TransferFunction.linear()``, made once (so that materials left at the default share one table)."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = TransferFunction.linear()
    return _DEFAULT
